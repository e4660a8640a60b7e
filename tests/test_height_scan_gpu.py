"""The terrain height scan on an MI355X (include/dyros_height_scan.h, csrc/dw_height_scan.hip): the HIP kernel against the
g++ build of the same header (tests/height_scan_host.cpp) bit for bit at the workgroup's edges, the wave's edges of P, every B and three maps,
with the output buffers too long and their tails watched; every way to choose outputs; the reference's lines run eagerly in torch on the same
device; a non-finite env; the plane under both tasks; the standing robots of the `borders` scene; a captured step plus refresh; a live env on
the default trimesh terrain with the key on and off; the player's files.

The grid channels (heights, points, obs) are the g++ build's bits under both rules and both gpu_div.  The probe channels are not: the chain
takes sinf / cosf of every joint's half angle, which the device computes with its own polynomial (ocml) and glibc with another, each within
an ulp, and terrain_sample's normal takes 1 / sqrt by v_rsq_f32 and a Newton step on the device, 1.0f / sqrtf on the host (dw_physics.h
rsqrt_nr).  Those channels are held within 4 d of float64 instead (normals away from lines), the rule of the CPU tests."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import height_scan_ref as R
import terrain_edge_cases as TE
from isaacgymdyros_amd import height_scan as H
from isaacgymdyros_amd.model import load_model
from test_height_scan import GOLD, OUTPUTS, SOLES, bits, check_against_float64, gold_case, host, host_scan, host_table, line_cases  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = H.GROUP          # envs per workgroup
PAD = 64
F = np.float32
K = H.K
NAN_BITS = 0x7fc00000
GRID_CHANNELS, PROBE_CHANNELS = OUTPUTS[:3], OUTPUTS[3:]


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def api():
    return H.declare(__import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0])


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scan(api, table, root, dof, hs, hscale=0.1, vscale=0.005, border=0.0, rule=0, gpu_div=0, want=OUTPUTS, expect=0, table_offset=0):
    """dwh_scan on numpy inputs; the outputs are PAD words too long and NaN-filled, and every word past the end must come back untouched.
    Returns the requested outputs as numpy arrays."""
    n, P, B = len(root), int(table[K["DWH_T_NP"]]), int(table[K["DWH_T_NB"]])
    dof = np.zeros((n, 33, 2), F) if dof is None else dof
    words = dict(heights=n * P, points=n * P * 2, obs=n * P, probe_pos=n * B * 3, probe_height=n * B, clearance=n * B, probe_normal=n * B * 3)
    shapes = dict(heights=(n, P), points=(n, P, 2), obs=(n, P), probe_pos=(n, B, 3), probe_height=(n, B), clearance=(n, B), probe_normal=(n, B, 3))
    d = [dev(np.concatenate([np.zeros(table_offset, np.int32), table.view(np.int32)])), dev(np.ascontiguousarray(root, F)), dev(np.ascontiguousarray(dof, F)),
         None if hs is None else dev(np.ascontiguousarray(hs, np.int16))]
    out = {k: torch.full((words[k] + PAD,), float("nan"), device=DEV) for k in want}
    rows, cols = (0, 0) if hs is None else hs.shape
    rc = api["scan"](n, d[0].data_ptr() + 4 * table_offset, d[1].data_ptr(), d[2].data_ptr(), None if hs is None else d[3].data_ptr(), rows, cols, hscale,
                     vscale, border, rule, gpu_div, *[out[k].data_ptr() if k in out else None for k in OUTPUTS], stream())
    torch.cuda.synchronize()          # (d is freed after this)
    assert rc == expect, api["last_error"]()
    res = {}
    for k, t in out.items():
        h = t.cpu().numpy()
        assert (h[words[k]:].view(np.uint32) == NAN_BITS).all(), (k, np.argwhere(h[words[k]:].view(np.uint32) != NAN_BITS)[:5])
        res[k] = h[:words[k]].reshape(shapes[k]) if rc == 0 else h
    return res


def inputs(which, n):
    """(field arguments, root, dof) of n seeded envs on one of the three maps: 70 x 90 (`borders`), 33 x 27 (`scales_h0.25`), 2 x 2."""
    if which == "2x2":
        field = TE.Field(GOLD["field_tiny"], 0.1, 0.005, 0.0)
        return (field,) + R.seeded_cases(field, seed=4300 + n, n=n)          # (every point clamps to the one cell)
    field, root, dof, _ = TE.scene({"70x90": "borders", "33x27": "scales_h0.25"}[which])
    return field, np.resize(root, (n, 13)), np.resize(dof, (n, 33, 2))


def fargs(field):
    return field.heightsamples, field.hscale, field.vscale, field.border


CAP_GRID = H.mesh(np.linspace(-1.55, 1.55, 32), np.linspace(-1.55, 1.55, 32))


def grid_of(P):
    return CAP_GRID if P == K["DWH_MAX_POINTS"] else np.resize(GOLD["grid"], (P, 2))


def probes_of(B):
    names = load_model().body_names
    more = [{"body": names[g], "gym": g, "pos": [0.05, -0.02, 0.03]} for g in (0, 29, 37, 22, 3, 11, 14, 33)]          # base, head, hands, legs, waist
    return (SOLES + more)[:B] if B != 1 else [more[2]]


# ---------------------------------------------------------------------------------------------- the kernel against the g++ build
@pytest.mark.parametrize("which,n,P,B", [("70x90", 1, 140, 8), ("70x90", G - 1, 63, 1), ("70x90", G, 64, 0), ("70x90", G + 1, 65, 16), ("70x90", 14, 1, 8),
                                         ("70x90", 3 * G + 5, K["DWH_MAX_POINTS"], 8), ("33x27", G + 1, 140, 16), ("33x27", 14, 64, 0),
                                         ("2x2", G + 1, 140, 8), ("2x2", 1, 1, 1)])
def test_kernel_equals_the_host_build(api, host, which, n, P, B):
    """n: one env, the group's edge, 14 and three groups and a part; P: one point, the wave's edge, the default and the cap; B: none, one, the soles,
    the cap.  Both rules and both gpu_div."""
    field, root, dof = inputs(which, n)
    grid, probes = grid_of(P), probes_of(B)
    t = host_table(host, grid, probes, obs={"offset": 0.5, "clip": 1.0, "scale": 5.0})
    d = R.channel_d(field, t, GOLD["grid"], probes, (which, B)) if B else None
    for rule in (0, 1):
        for gpu_div in (0, 1):
            want = host_scan(host, t, root, dof, *fargs(field), rule, gpu_div)
            got = scan(api, t, root, dof, *fargs(field), rule, gpu_div)
            for k in GRID_CHANNELS:
                assert np.array_equal(bits(got[k]), bits(want[k])), (k, rule, gpu_div, int((bits(got[k]) != bits(want[k])).sum()))
            if B:
                print("%s n=%d P=%d B=%d rule=%d div=%d: words that differ from the g++ build: %s" % (
                    which, n, P, B, rule, gpu_div, {k: int((bits(got[k]) != bits(want[k])).sum()) for k in PROBE_CHANNELS}))
                check_against_float64(field, root, dof, grid, probes, {k: got[k] for k in PROBE_CHANNELS}, d, which)
            else:
                assert all((bits(got[k]) == NAN_BITS).all() for k in PROBE_CHANNELS)          # B = 0: the probe outputs are not touched


@pytest.mark.parametrize("gpu_div", (0, 1))
def test_kernel_on_sample_lines(api, host, gpu_div):
    field = TE.scene("lines")[0]
    root, grid = line_cases(field)
    t = host_table(host, grid, obs={})
    for rule in (0, 1):
        want = host_scan(host, t, root, None, *fargs(field), rule, gpu_div, GRID_CHANNELS)
        got = scan(api, t, root, None, *fargs(field), rule, gpu_div, GRID_CHANNELS)
        for k in GRID_CHANNELS:
            assert np.array_equal(bits(got[k]), bits(want[k])), (k, rule)


def test_every_output_alone_and_all_but_it(api, host):
    field, root, dof = inputs("70x90", G + 3)
    t = host_table(host, GOLD["grid"], SOLES, obs={})
    full = scan(api, t, root, dof, *fargs(field), 0, 1)
    for k in OUTPUTS:
        one = scan(api, t, root, dof, *fargs(field), 0, 1, (k,))
        rest = scan(api, t, root, dof, *fargs(field), 0, 1, tuple(o for o in OUTPUTS if o != k))
        assert list(one) == [k] and np.array_equal(bits(one[k]), bits(full[k])), k
        assert all(np.array_equal(bits(rest[o]), bits(full[o])) for o in rest), k
    # a table 4 bytes past a 16-byte boundary is refused, and nothing was launched: the buffer still holds its fill
    res = scan(api, t, root, dof, *fargs(field), 0, 1, ("heights",), expect=-1, table_offset=1)
    assert b"16-byte aligned" in api["last_error"]() and (res["heights"].view(np.uint32) == NAN_BITS).all()


# ---------------------------------------------------------------------------------------------- the reference's lines on the same device
def test_kernel_equals_the_torch_twin_on_the_device(api, host):
    t = host_table(host, GOLD["grid"])
    pts = torch.zeros(16, 140, 3, device=DEV)
    pts[:, :, :2] = dev(GOLD["grid"])
    inside = total = 0
    for c in range(len(GOLD["root"])):
        hs, hscale, vscale, border = gold_case(c)
        root = GOLD["root"][c]
        got = scan(api, t, root, None, hs, hscale, vscale, border, 0, 1, ("heights",))["heights"]
        twin = R.torch_twin(dev(root), pts, dev(hs), border, hscale, vscale).cpu().numpy()
        near = R.near_line(*R.coords64(root, GOLD["grid"], border, hscale), R.d_u_of(root, GOLD["grid"], border, hscale, 1))
        assert np.array_equal(bits(got)[~near], bits(twin)[~near]), (c, int((bits(got) != bits(twin))[~near].sum()))
        inside, total = inside + int(near.sum()), total + near.size
    print("torch twin on the device: %d of %d points inside the near-line band (not held)" % (inside, total))
    assert inside <= R.NEAR_CAP * total


def test_kernel_equals_the_recorded_reference(api, host):
    """With gpu_div = 0 the kernel gives the reference's recorded heights and observation line at every point of the fixture, the 282 near
    sample lines included (two envs stand on lines with yaw 0: the points that tell how the reference divides)."""
    from test_height_scan import OBS
    t = host_table(host, GOLD["grid"], obs=dict(zip(("offset", "clip", "scale"), OBS)))
    for c in range(len(GOLD["root"])):
        got = scan(api, t, GOLD["root"][c], None, *gold_case(c), 0, 0, ("heights", "obs"))
        assert np.array_equal(bits(got["heights"]), bits(GOLD["heights"][c])) and np.array_equal(bits(got["obs"]), bits(GOLD["obs"][c])), c


# ---------------------------------------------------------------------------------------------- a non-finite env
def test_a_non_finite_env_gets_nan_and_its_neighbours_keep_their_bits(api, host):
    field, root, dof = inputs("70x90", 2 * G + 3)
    t = host_table(host, GOLD["grid"], SOLES, obs={})
    ref = scan(api, t, root, dof, *fargs(field), 1, 1)
    bad_root, bad_dof = root.copy(), dof.copy()
    bad_root[3, 11], bad_root[G, 0], bad_dof[G + 5, 20, 0], bad_dof[2 * G + 2, 4, 0] = np.inf, np.nan, np.nan, -np.inf
    bad = [3, G, G + 5, 2 * G + 2]
    got = scan(api, t, bad_root, bad_dof, *fargs(field), 1, 1)          # (the tails are watched in scan())
    for k in OUTPUTS:
        assert np.isnan(got[k][bad]).all() and np.array_equal(bits(np.delete(got[k], bad, 0)), bits(np.delete(ref[k], bad, 0))), k


# ---------------------------------------------------------------------------------------------- the standing robots
def test_standing_robots_are_inside_the_ground(api, host):
    """The `borders` scene places every robot with its deepest sole corner 0.1 .. 4 mm inside the ground: the lowest clearance is negative for
    every env and within 4 d of the float64 gap."""
    field, root, dof, _ = TE.scene("borders")
    t = host_table(host, GOLD["grid"], SOLES)
    d = R.channel_d(field, t, GOLD["grid"], SOLES, "borders")
    clr = scan(api, t, root, dof, *fargs(field), 1, 1, ("clearance",))["clearance"]
    c = TE.sole_corners(root, dof[:, :, 0])
    gap = c[:, :, 2] - field.height_at(c[:, :, 0], c[:, :, 1])
    err = float(np.abs(clr.min(axis=1) - gap.min(axis=1)).max())
    print("lowest corner against the float64 gap: err %.3e, 4 d = %.3e; lowest clearance %.4f .. %.4f m" % (err, 4 * d["clearance"], clr.min(1).min(), clr.min(1).max()))
    assert err <= 4 * d["clearance"] and (clr.min(axis=1) < 0).all() and clr.min() > -0.0045


# ---------------------------------------------------------------------------------------------- envs
def make_env(n, spec=None, terrain=None, **mi):
    from isaacgymdyros_amd.config import default_cfg, with_terrain
    from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk
    cfg = default_cfg(n, DEV)
    if terrain:
        cfg = with_terrain(cfg, mesh_type=terrain)
    cfg["seed"] = 42
    cfg["env"]["episodeLength"] = 0.1          # (seconds; 0.004 s per policy step: every env meets the time limit at step 25)
    cfg["sim"]["mi355"]["device_step_counter"] = True
    cfg["sim"]["mi355"]["alias_obs"] = True
    cfg["sim"]["mi355"].update(mi)
    if spec is not None:
        cfg["sim"]["mi355"]["height_scan"] = spec
    return DyrosDynamicWalk(cfg, DEV, 0, True)


def actions(n, steps, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    amp = torch.tensor([0.0, 0.05, 0.3, 1.0], device=DEV)[torch.arange(n, device=DEV) % 4].view(1, n, 1)
    return ((torch.rand(steps, n, 13, generator=g, device=DEV) * 2 - 1) * amp).contiguous()


def tbits(*ts):
    return torch.cat([t.reshape(-1).view(torch.int32) if t.dtype == torch.float32 else t.reshape(-1).to(torch.int32) for t in ts])


def test_the_plane_under_both_tasks():
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    n = 32
    env = make_env(n, {"normals": True, "obs": {}, "points": True})
    a = actions(n, 5)
    for i in range(5):
        env.step(a[i].clone())
    hs = env.height_scan
    h = env.get_heights()
    assert h is hs.heights and h.shape == (n, 140) and not h.view(torch.int32).any()          # +0.0
    assert torch.equal(hs.clearance.view(torch.int32), hs.probe_pos[..., 2].contiguous().view(torch.int32)) and not hs.probe_heights.view(torch.int32).any()
    assert (hs.probe_normals == torch.tensor([0.0, 0.0, 1.0], device=DEV)).all() and hs.names == [p["body"] for p in SOLES]
    assert torch.equal(hs.obs, torch.clip(env.root_states[:, 2:3] - 0.5 - h, -1.0, 1.0)) and torch.isfinite(hs.points).all()
    env.close()
    cfg = default_amp_cfg(n, DEV)
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert amp.height_scan is None
    with pytest.raises(RuntimeError):
        amp.get_heights()
    amp.close()
    cfg = default_amp_cfg(n, DEV)
    cfg["sim"].setdefault("mi355", {})["amp_height_scan"] = {"auto": True}
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert isinstance(amp.height_scan, H.HeightScan) and amp._phys.height_scan is None
    g = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(5):
        amp.step((torch.rand(n, amp.num_actions, generator=g, device=DEV) * 2 - 1) * 0.1)
    hs = amp.height_scan
    held = hs.clearance.clone()
    assert amp.get_heights().shape == (n, 140) and not hs.heights.view(torch.int32).any()
    assert torch.equal(held, hs.clearance) and torch.equal(hs.clearance, hs.probe_pos[..., 2]) and float(hs.clearance.min()) > -0.05
    amp.close()


def test_captured_step_plus_refresh_replays_the_eager_bits():
    """Step and refresh recorded in one graph on one stream (a linear chain), replayed 10 times, against 10 eager steps from the same state."""
    n = 64
    acts = actions(n, 11, seed=3)
    outs = []
    for captured in (False, True):
        env = make_env(n, {"auto": True, "obs": {}, "normals": True}, terrain="heightfield")
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
        for i in range(1, 11):
            a.copy_(acts[i])
            if captured:
                g.replay()
            else:
                env.step(a)
            hs = env.height_scan
            h.append(tbits(hs.heights, hs.obs, hs.clearance, hs.probe_normals, env._buf["root_states"]))
        torch.cuda.synchronize()
        outs.append(torch.stack(h).cpu())
        env.close()
    assert torch.equal(outs[0], outs[1]) and len(torch.unique(outs[0][-1][:n * 140])) > 2          # (and the heights are a field's, not the plane's)


def test_live_env_on_the_default_trimesh_terrain(api, host):
    """40 steps on with_terrain(default_cfg(64), mesh_type="trimesh"): observations and rewards are the same bits with the key on ("auto") or
    absent; what the env's scan holds is the C ABI's answer on the env's own buffers and the torch twin's away from lines."""
    n, steps = 64, 40
    acts = actions(n, steps)
    runs = {}
    for name, spec in (("off", None), ("auto", {"auto": True})):
        env = make_env(n, spec, terrain="trimesh")
        a, h = torch.zeros(n, 13, device=DEV), []
        if spec is None:
            assert env.height_scan is None
            with pytest.raises(RuntimeError):
                env.get_heights()
        for i in range(steps):
            a.copy_(acts[i])
            o, r, d, _ex = env.step(a)
            h.append(tbits(o["obs"], r, d, env._buf["root_states"]))
        if spec is not None:
            hs, c = env.height_scan, env._ccfg
            assert hs.heights.shape == (n, 140) and hs.clearance.shape == (n, 8) and hs.probe_normals is None and hs.points is None and hs.obs is None
            root, dof = env._buf["root_states"].cpu().numpy(), env._buf["dof_state"].cpu().numpy()
            samples = env.height_samples.cpu().numpy()
            assert samples.shape == (c.terrain_rows, c.terrain_cols) and samples.dtype == np.int16
            margs = (samples, float(c.terrain_hscale), float(c.terrain_vscale), float(c.terrain_border))
            again = scan(api, host_table(host, hs.grid, SOLES), root, dof, *margs, 0, hs.gpu_div, ("heights", "clearance", "probe_pos"))
            assert np.array_equal(bits(hs.heights.cpu().numpy()), bits(again["heights"])) and np.array_equal(bits(hs.clearance.cpu().numpy()), bits(again["clearance"]))
            pts = torch.zeros(n, 140, 3, device=DEV)
            pts[:, :, :2] = dev(hs.grid)
            twin = R.torch_twin(env._buf["root_states"], pts, env.height_samples, margs[3], margs[1], margs[2]).cpu().numpy()
            near = R.near_line(*R.coords64(root, hs.grid, margs[3], margs[1]), R.d_u_of(root, hs.grid, margs[3], margs[1], 1))
            print("live env: %d of %d points near a line; lowest sole clearance %.4f m; heights %.3f .. %.3f m" % (
                int(near.sum()), near.size, float(hs.clearance.min()), float(hs.heights.min()), float(hs.heights.max())))
            assert hs.gpu_div == 1 and near.mean() <= R.NEAR_CAP and np.array_equal(bits(hs.heights.cpu().numpy())[~near], bits(twin)[~near])
            assert -0.05 < float(hs.clearance.min(dim=1).values.median()) < 0.3          # the robots are at the ground the scan sees, not metres off it
            env.reset_idx(torch.arange(0, n, 2, device=DEV))          # reset_idx refreshes too
            assert torch.equal(hs.probe_pos, torch.from_numpy(scan(api, host_table(host, hs.grid, SOLES), env._buf["root_states"].cpu().numpy(),
                                                                   env._buf["dof_state"].cpu().numpy(), *margs, 0, 1, ("probe_pos",))["probe_pos"]).to(DEV))
        runs[name] = torch.stack(h).cpu()
        env.close()
    assert torch.equal(runs["off"], runs["auto"])


# ---------------------------------------------------------------------------------------------- the player
def test_player_writes_the_scans(tmp_path):
    import importlib.util
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
    out = tmp_path / "scan"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "examples", "ppo_player.py"), "--checkpoint", ck, "--num-envs", "64",
                        "--games", "64", "--max-steps", "60", "--episode-length", "0.1", "--scan-dir", str(out), "--scan-envs", "2"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["scan_env0.npz", "scan_env1.npz"]
    z = np.load(out / "scan_env1.npz")
    T = z["heights"].shape[0]
    assert 20 <= T <= 60 and z["grid"].shape == (140, 2) and z["heights"].shape == (T, 140) and z["probe_pos"].shape == (T, 8, 3)
    assert z["clearance"].shape == (T, 8) and float(z["dt"]) == pytest.approx(0.004) and z["names"].tolist() == [p["body"] for p in SOLES]
    assert np.array_equal(bits(z["grid"]), bits(GOLD["grid"])) and not z["heights"].any() and np.array_equal(z["clearance"], z["probe_pos"][..., 2])
