"""The motion library on the device (cfg sim.mi355.amp_motion_device; include/dyros_walk.h dw_amp_motion_state / _obs, dw_amp_reset_rows_motion,
dw_amp_reset_done_motion; csrc/dw_amp_motion.h) against the host path it replaces: get_motion_state and _motion_amp_obs query by query, the
class with the caller's draws against the class without the key call by call, the device draws against their numpy restatement
(tests/amp_motion_ref.py).  Shapes: 37 envs (more than one 16-env group, not a multiple of one), three motions of unequal length and weight,
one played backwards, numAMPObsSteps 2 and 4."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import amp_motion_ref as MR

pytestmark = pytest.mark.gpu
N = 37
TRANS_AMP = [1, 2, 3, 28, 29, 30, 31, 32, 33]          # words of a discriminator observation behind atan2 / the heading frame
COPY_AMP = [0] + list(range(4, 28))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module")
def motions(tmp_path_factory):
    from isaacgymdyros_amd.motion_lib import TocabiLowerMotionLib
    tmp = str(tmp_path_factory.mktemp("motions"))
    yml, one = MR.write_small(tmp), MR.write_slerp_table(tmp)
    return {"yml": yml, "small": TocabiLowerMotionLib(yml, 33, "cuda:0"), "slerp": TocabiLowerMotionLib(one, 33, "cuda:0")}


@pytest.fixture(scope="module")
def api():
    from isaacgymdyros_amd import _lib
    return _lib.load()[1]


def _queries(motions, which):
    lib = motions[which]
    if which == "small":
        return MR.queries(lib)
    dt = abs(float(lib._motion_dt[0]))
    times = np.array([(k + f) * dt for k in range(5) for f in (0.0, 0.25, 0.5, 0.8125)] + [-0.3 * dt, 5 * dt])
    return np.zeros(len(times), dtype=np.int64), times


def _dev(ids, times):
    return torch.tensor(ids, dtype=torch.int32, device="cuda"), torch.tensor(times, dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("which", ["small", "slerp"])
def test_motion_state_equals_get_motion_state(motions, api, which):
    """Joint state, velocities and the lerped positions bit for bit; the root rotation bit for bit through slerp's identical and nearly
    parallel branches and to atol 2e-6 (the bound test_tocabi_amp_lower_reference_state_init holds that quantity to) through its general one:
    acosf / sinf of the device library against torch's kernels."""
    lib = motions[which]
    tab = lib.device_table()
    ids, times = _queries(motions, which)
    n = len(ids)
    rp, rr, rv, ra, dp, dv, kp = lib.get_motion_state(ids, times)
    mi, mt = _dev(ids, times)
    root, dpos, dvel, key = (torch.full((n, w), float("nan"), device="cuda") for w in (13, 12, 12, 6))
    rc = api["amp_motion_state"](C.byref(tab.struct()), n, _p(mi), _p(mt), _p(root), _p(dpos), _p(dvel), _p(key), 1, None)
    assert rc == 0, api["last_error"]()
    torch.cuda.synchronize()
    assert torch.equal(dpos, dp) and torch.equal(dvel, dv)
    assert torch.equal(root[:, 0:3], rp) and torch.equal(root[:, 7:10], rv) and torch.equal(root[:, 10:13], ra)
    assert torch.equal(key.view(n, 2, 3), kp)
    br, neg = MR.slerp_branch(MR.HostTable(tab), ids, times)
    if which == "slerp":
        assert (br == 0).any() and (br == 1).any() and ((br == 2) & neg).any() and ((br == 2) & ~neg).any()
    exact = torch.tensor(br < 2, device="cuda")
    assert torch.equal(root[exact, 3:7], rr[exact])
    err = float((root[:, 3:7] - rr).abs().max())
    print("dw_amp_motion_state[%s]: root rotation, max |difference| through slerp's general branch: %.3g" % (which, err))
    assert err <= 2e-6


@pytest.mark.parametrize("steps", [2, 4])
def test_motion_obs_equals_the_class_function(motions, api, steps):
    """dw_amp_motion_obs against _motion_amp_obs (get_motion_state + dw_amp_disc_observations) with first_k 0 (fetch_amp_obs_demo) and 1 (the
    history of a reference start): copies bit for bit, Euler angles and heading-frame words to the 2e-5 of the existing test."""
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    cfg = default_amp_cfg(N, "cuda:0")
    cfg["env"].update({"stateInit": "Random", "motion_file": motions["yml"], "numAMPObsSteps": steps})
    env = TocabiAMPLower(cfg, "cuda:0", 0, True)
    tab = env._motion_lib.device_table()
    ids, times0 = MR.queries(env._motion_lib)
    n = len(ids)
    mi, mt = _dev(ids, times0)
    for first_k, ns in ((0, steps), (1, steps - 1)):
        mids = np.tile(np.expand_dims(ids, axis=-1), [1, ns]).flatten()
        times = (np.expand_dims(times0, axis=-1) + (-env.dt * (np.arange(0, ns) + first_k))).flatten()
        ref = env._motion_amp_obs(mids, times).view(n, ns, 34)
        out = torch.full((n, ns, 34), float("nan"), device="cuda")
        rc = api["amp_motion_obs"](C.byref(tab.struct()), n, ns, _p(mi), _p(mt), float(env.dt), first_k, 0, _p(out), 1, None)
        assert rc == 0, api["last_error"]()
        torch.cuda.synchronize()
        assert torch.equal(out[..., COPY_AMP], ref[..., COPY_AMP]), first_k
        err = float((out[..., TRANS_AMP] - ref[..., TRANS_AMP]).abs().max())
        print("dw_amp_motion_obs steps %d first_k %d: max |difference| of the Euler / heading-frame words: %.3g" % (ns, first_k, err))
        assert err <= 2e-5
    env.close()


# ------------------------------------------------------------------------------------------------ class level, the caller's draws
OBS_TRANS = list(range(9))          # words of the 36-word observation behind the root rotation (Euler angles, velocities in the root frame)


def _split_obs(env, x):
    """(exact part, part downstream of the root rotation) of a stacked observation [N, num_obs]"""
    H = env.num_obs_his
    o = x[:, :36 * H].reshape(x.shape[0], H, 36)
    rest = torch.ones(36, dtype=torch.bool)
    rest[OBS_TRANS] = False
    return torch.cat([o[..., rest].reshape(x.shape[0], -1), x[:, 36 * H:]], dim=1), o[..., OBS_TRANS]


def _compare(a, b, where):
    """a: with amp_motion_device, b: without.  Integer state, everything made of uniforms, the Gym tensors and every copied word bit for
    bit; the words behind slerp / atan2 / the heading frame to the tolerances of the kernel tests."""
    for n in ("progress_buf", "reset_buf", "_terminate_buf", "randomize_buf", "perturb_timing", "delay_idx", "simul_len", "vel_change_duration",
              "cur_vel_change_duration", "commands", "qpos_bias", "quat_bias", "power_scale", "epi_len", "epi_len_log", "qpos_noise", "qpos_pre",
              "qvel_noise", "_dof_vel_pre", "actions_pre", "action_log", "_dof_state", "_root_states", "_contact_forces", "rew_buf"):
        assert torch.equal(getattr(a, n), getattr(b, n)), (where, n)
    for n in ("dof_damping", "dof_armature"):
        assert torch.equal(a._phys._buf[n], b._phys._buf[n]), (where, n)
    (aa, ao), (ba, bo) = a.history_linear(), b.history_linear()
    assert torch.equal(aa, ba), (where, "action_history")
    rest = torch.ones(36, dtype=torch.bool)
    rest[OBS_TRANS] = False
    ao, bo = ao.view(N, -1, 36), bo.view(N, -1, 36)
    assert torch.equal(ao[..., rest], bo[..., rest]), (where, "obs_history")
    worst = float((ao[..., OBS_TRANS] - bo[..., OBS_TRANS]).abs().max())
    for x, y in ((a.obs_buf, b.obs_buf), (a.obs_dict["obs"], b.obs_dict["obs"])):
        (xe, xt), (ye, yt) = _split_obs(a, x), _split_obs(b, y)
        assert torch.equal(xe, ye), (where, "obs")
        worst = max(worst, float((xt - yt).abs().max()))
    assert torch.equal(a._amp_obs_buf[..., COPY_AMP], b._amp_obs_buf[..., COPY_AMP]), (where, "amp_obs_buf")
    worst = max(worst, float((a._amp_obs_buf[..., TRANS_AMP] - b._amp_obs_buf[..., TRANS_AMP]).abs().max()))
    worst = max(worst, float((a._foot_pos - b._foot_pos).abs().max()))
    assert worst <= 2e-5, (where, worst)
    return worst


@pytest.mark.parametrize("form", ["fused_ring", "fused_shifting", "fused_reset_alone"])
@pytest.mark.parametrize("mode,steps", [("Start", 2), ("Random", 4), ("Hybrid", 2)])
def test_class_with_the_callers_draws_equals_the_torch_reset(motions, mode, steps, form):
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    envs = []
    for key in (True, False):
        cfg = default_amp_cfg(N, "cuda:0")
        # (a 12-step episode: every env resets three times in the 40 steps whatever the actions do -- besides the falls of the motion starts,
        #  whose synthetic leg poses lift a foot above the termination height)
        cfg["env"].update({"episodeLength": 12, "stateInit": mode, "hybridInitProb": 0.5, "numAMPObsSteps": steps, "motion_file": motions["yml"]})
        mi = {"amp_fused_reset": True} if form == "fused_reset_alone" else {"amp_fused": True}
        if form == "fused_shifting":
            mi["amp_hist_ring"] = False
        if not key:
            mi.pop("amp_fused_reset", None)          # (without the key a motion start leaves the fused reset anyway)
        else:
            mi["amp_motion_device"] = True
        cfg["sim"]["mi355"] = mi
        envs.append(TocabiAMPLower(cfg, "cuda:0", 0, True))
    a, b = envs
    assert a._motion_device and not b._motion_device and a._hist_ring == (form == "fused_ring") and not b._hist_ring
    g = torch.Generator(device="cuda").manual_seed(11)
    st = [np.random.RandomState(5).get_state()] * 2
    n_motion = n_default = later = 0
    worst = 0.0
    for t in range(40):
        out = []
        for k, e in enumerate((a, b)):
            np.random.set_state(st[k])
            out.append(e.reset_done())
            st[k] = np.random.get_state()
        ids = out[0][1]
        assert torch.equal(ids, out[1][1]), t
        if len(ids) > 0:
            assert torch.equal(torch.as_tensor(a._reset_ref_env_ids), torch.as_tensor(b._reset_ref_env_ids)), t
            assert torch.equal(torch.as_tensor(a._reset_default_env_ids), torch.as_tensor(b._reset_default_env_ids)), t
            assert np.array_equal(a._reset_ref_motion_ids, b._reset_ref_motion_ids) and np.array_equal(a._reset_ref_motion_times, b._reset_ref_motion_times), t
            ref_now = set(ids.tolist()) & set(torch.as_tensor(b._reset_ref_env_ids).tolist())
            n_motion += len(ref_now)
            n_default += len(ids) - len(ref_now)
            later += t > 0
        worst = max(worst, _compare(a, b, (t, "reset_done")))
        act = (torch.rand(N, 12, generator=g, device="cuda") * 2 - 1) * 0.7
        oa, ra, da, xa = a.step(act)
        ob, rb, db, xb = b.step(act)
        assert torch.equal(ra, rb) and torch.equal(da, db), t
        worst = max(worst, _compare(a, b, (t, "step")))
    print("%s / %s / %d steps: max |difference| of the words behind slerp, atan2 and the heading frame: %.3g; %d motion and %d default starts"
          % (mode, form, steps, worst, n_motion, n_default))
    assert n_motion >= 1 and later >= 2
    if mode == "Hybrid":
        assert n_default >= 1
    for e in envs:
        e.close()


# ------------------------------------------------------------------------------------------------ the device's draws
def _device_env(motions, seed, steps=2, graph=False):
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    cfg = default_amp_cfg(N, "cuda:0")
    cfg["seed"] = seed
    cfg["env"].update({"episodeLength": 12, "stateInit": "Hybrid", "hybridInitProb": 0.5, "numAMPObsSteps": steps, "motion_file": motions["yml"]})
    cfg["sim"]["mi355"] = {"amp_fused": True, "amp_device_draws": True, "amp_motion_device": True}
    env = TocabiAMPLower(cfg, "cuda:0", 0, True)
    assert env._hist_ring and env._device_draws
    if graph:
        env.reset_done()
        env.enable_graph_step(warmup=2)
    return env


def test_device_draws_equal_their_numpy_restatement(motions):
    """Kinds, motions and times of dw_amp_reset_done_motion against tests/amp_motion_ref.device_start_draws: the integers equal, the times equal
    AS FLOAT64 (the phase-to-time product is float64(uniform) * length in float64 on both sides); the draw counters equal this test's own
    count (one per step, one per reset); a motion start carries the table's joint state and its history the motion's earlier frames."""
    env = _device_env(motions, 21, steps=4)
    tab = MR.HostTable(env._motion_tab)
    count = np.zeros(N, dtype=np.int64)
    seen = {0: 0, 1: 0}
    for t in range(30):
        assert np.array_equal(env._draw_ctr.cpu().numpy(), count), t
        kind, motion, time = MR.device_start_draws(tab, 21, N, count, "Hybrid", 0.5)
        _, ids = env.reset_done()
        i = ids.cpu().numpy()
        dk, dm, dtm = (x.cpu().numpy() for x in env._drawn_start)
        assert np.array_equal(dk[i], kind[i]), t
        ref = i[kind[i] == 1]
        assert np.array_equal(dm[ref], motion[ref]) and np.array_equal(dtm[ref], time[ref]), t
        assert (dm[i[kind[i] == 0]] == -1).all()
        seen[0] += int((kind[i] == 0).sum()); seen[1] += len(ref)
        count[i] += 1
        if len(ref) > 0:
            r = torch.as_tensor(ref, device="cuda")
            _, _, _, _, dp, dv, _ = MR.motion_state(tab, motion[ref], time[ref])
            assert torch.equal(env._dof_pos[r, :12].cpu(), dp) and torch.equal(env._dof_vel[r, :12].cpu(), dv), t
            assert torch.equal(env._dof_pos[r, 12:], env._initial_dof_pos[r, 12:]) and torch.equal(env._root_states[r], env._initial_root_states[r])
            for k in (1, 2, 3):
                rp, _, _, _, dp, dv, _ = MR.motion_state(tab, motion[ref], time[ref] + (-env.dt * k))
                h = env._amp_obs_buf[r, k].cpu()
                assert torch.equal(h[:, 0], rp[:, 2]) and torch.equal(h[:, 4:16], dp) and torch.equal(h[:, 16:28], dv), (t, k)
        d = torch.as_tensor(i[kind[i] == 0], device="cuda")
        assert torch.equal(env._amp_obs_buf[d, 1:], env._amp_obs_buf[d, :1].expand(-1, 3, -1)) and torch.equal(env._dof_pos[d], env._initial_dof_pos[d])
        env.step(torch.zeros(N, 12, device="cuda"))
        count += 1
    assert seen[0] >= 10 and seen[1] >= 10
    env.close()


def test_device_draws_under_graph_replay(motions):
    """step() replayed from a hipGraph with reset_done() between the replays: the same seed gives the same run, another seed another, and an
    env's successive resets draw different starts (the draw counters live in device memory)."""
    a, b, c = _device_env(motions, 3, graph=True), _device_env(motions, 3, graph=True), _device_env(motions, 4, graph=True)
    g = torch.Generator(device="cuda").manual_seed(2)
    starts = []
    for t in range(30):
        ids = [e.reset_done()[1] for e in (a, b, c)]
        assert torch.equal(ids[0], ids[1]), t
        for x, y in zip(a._drawn_start, b._drawn_start):
            assert torch.equal(x, y), t
        assert torch.equal(a._amp_obs_buf, b._amp_obs_buf) and torch.equal(a._dof_state, b._dof_state), t
        if len(ids[0]) > 0:
            starts.append((ids[0].clone(), a._drawn_start[0].clone(), a._drawn_start[2].clone()))
        act = (torch.rand(N, 12, generator=g, device="cuda") * 2 - 1) * 0.6
        oa, ob = a.step(act)[0]["obs"], b.step(act)[0]["obs"]
        c.step(act)
        assert torch.equal(oa, ob), t
    assert not torch.equal(a._drawn_start[2], c._drawn_start[2])
    assert len(starts) >= 2 and not torch.equal(starts[0][2], starts[-1][2]) and not torch.equal(starts[0][1], starts[-1][1])
    for e in (a, b, c):
        e.close()


def test_motion_argument_checks(motions, api):
    """Every refusal comes back as an error code with dw_last_error() set; nothing is launched."""
    env = _device_env(motions, 1)
    tab, h = env._motion_tab.struct(), env._phys._h
    c, b = env._fused_tables()
    n = 5
    mi, mt = _dev(np.array([0, 1, 2, 1, 0]), np.zeros(n))
    bad = torch.tensor([0, 1, 3, 1, 0], dtype=torch.int32, device="cuda")
    root, dp, dv, key = (torch.zeros(n, w, device="cuda") for w in (13, 12, 12, 6))
    out = torch.zeros(n, 2, 34, device="cuda")
    ids = torch.arange(n, device="cuda")
    u = torch.rand(N, 12, device="cuda")
    i64 = torch.ones(n, dtype=torch.int64, device="cuda")
    from isaacgymdyros_amd import abi
    notab = abi.DwMotionTable()
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)

    def refused(what, rc):
        msg = api["last_error"]().decode()
        assert rc != 0 and what in msg, (what, rc, msg)
    T = C.byref(tab)
    state = lambda *a: api["amp_motion_state"](*a)
    refused("dw_amp_motion_state", state(None, n, _p(mi), _p(mt), _p(root), _p(dp), _p(dv), _p(key), 1, None))
    refused("dw_amp_motion_state", state(C.byref(notab), n, _p(mi), _p(mt), _p(root), _p(dp), _p(dv), _p(key), 1, None))
    refused("dw_amp_motion_state", state(T, -1, _p(mi), _p(mt), _p(root), _p(dp), _p(dv), _p(key), 1, None))
    refused("dw_amp_motion_state", state(T, n, None, _p(mt), _p(root), _p(dp), _p(dv), _p(key), 1, None))
    refused("dw_amp_motion_state", state(T, n, _p(mi), _p(mt), _p(root), _p(dp), None, _p(key), 1, None))
    refused("misaligned", state(T, n - 1, _p(mi), off(mt, 4), _p(root), _p(dp), _p(dv), _p(key), 1, None))
    refused("misaligned", state(T, n - 1, off(mi, 2), _p(mt), _p(root), _p(dp), _p(dv), _p(key), 1, None))
    refused("motion id out of range", state(T, n, _p(bad), _p(mt), _p(root), _p(dp), _p(dv), _p(key), 1, None))
    obs = lambda *a: api["amp_motion_obs"](*a)
    refused("dw_amp_motion_obs", obs(None, n, 2, _p(mi), _p(mt), 0.002, 0, 0, _p(out), 1, None))
    refused("dw_amp_motion_obs", obs(T, -1, 2, _p(mi), _p(mt), 0.002, 0, 0, _p(out), 1, None))
    refused("steps < 1", obs(T, n, 0, _p(mi), _p(mt), 0.002, 0, 0, _p(out), 1, None))
    refused("dw_amp_motion_obs", obs(T, n, 2, _p(mi), _p(mt), 0.002, 0, 0, None, 1, None))
    refused("misaligned", obs(T, n - 1, 2, _p(mi), _p(mt), 0.002, 0, 0, off(out, 2), 1, None))
    refused("motion id out of range", obs(T, n, 2, _p(bad), _p(mt), 0.002, 0, 0, _p(out), 1, None))

    def rows(tabp=T, n_=n, m=mi, t=mt, hr=None, nhr=0, hm=None, ht=None, ids_=ids, c_=c):
        return api["amp_reset_rows_motion"](h, C.byref(c_), C.byref(b), tabp, _p(ids_), n_, None, _p(m), _p(t), _p(u), _p(u), _p(u), _p(u), _p(u), _p(u), _p(u),
                                            _p(i64), _p(i64), None, 0, _p(hr), nhr, _p(hm), _p(ht), 0.002, None)
    refused("dw_amp_reset_rows_motion", rows(tabp=None))
    refused("dw_amp_reset_rows_motion", rows(n_=-1))
    refused("dw_amp_reset_rows_motion", rows(m=None))
    refused("dw_amp_reset_rows_motion", rows(ids_=None))
    refused("history list", rows(hr=ids, nhr=n))
    refused("misaligned", api["amp_reset_rows_motion"](
        h, C.byref(c), C.byref(b), T, _p(ids), n - 1, None, _p(mi), off(mt, 4), _p(u), _p(u), _p(u), _p(u), _p(u), _p(u), _p(u), _p(i64), _p(i64), None, 0, None, 0,
        None, None, 0.002, None))
    refused("motion id out of range", rows(m=bad))
    refused("motion id out of range", rows(n_=0, hr=ids, nhr=n, hm=bad, ht=mt))
    done = lambda tabp, c_, si: api["amp_reset_done_motion"](h, C.byref(c_), C.byref(b), tabp, si, 0.5, 0.002, None, None, None, None)
    refused("dw_amp_reset_done_motion", done(None, c, 3))
    refused("state_init", done(T, c, 0))
    refused("state_init", done(T, c, 4))
    c2 = abi.DwAmpConfig.from_buffer_copy(c)
    c2.device_draws = 0
    refused("device_draws", done(T, c2, 3))
    c2 = abi.DwAmpConfig.from_buffer_copy(c)
    c2.amp_steps = 0
    refused("dw_amp_reset_done_motion", done(T, c2, 3))
    torch.cuda.synchronize()
    env.close()


def test_without_the_key_the_refusals_stand(motions):
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    for mi, match in (({"amp_fused": True, "amp_device_draws": True}, "amp_device_draws"), ({"amp_fused": True, "amp_hist_ring": True}, "amp_hist_ring")):
        cfg = default_amp_cfg(N, "cuda:0")
        cfg["env"].update({"stateInit": "Random", "motion_file": motions["yml"]})
        cfg["sim"]["mi355"] = mi
        with pytest.raises(ValueError, match=match):
            TocabiAMPLower(cfg, "cuda:0", 0, True)


@pytest.mark.parametrize("device_draws", [False, True])
def test_fetch_amp_obs_demo_on_the_device(motions, device_draws):
    """One launch into _amp_obs_demo_buf.  The caller's draws: numpy's generator as today, so the rows are those of the host path (copies bit
    for bit, the rest to 2e-5).  The device's: a torch.Generator on the device, reproducible from the seed, motions in the weights' proportions."""
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg

    def make(key):
        cfg = default_amp_cfg(N, "cuda:0")
        cfg["env"].update({"stateInit": "Random", "motion_file": motions["yml"], "numAMPObsSteps": 4})
        cfg["sim"]["mi355"] = {"amp_fused": True, "amp_motion_device": True, "amp_device_draws": device_draws} if key else {}
        return TocabiAMPLower(cfg, "cuda:0", 0, True)
    a = make(True)
    if not device_draws:
        b = make(False)
        np.random.seed(5)
        x = a.fetch_amp_obs_demo(301).view(301, 4, 34)
        np.random.seed(5)
        y = b.fetch_amp_obs_demo(301).view(301, 4, 34)
        assert torch.equal(x[..., COPY_AMP], y[..., COPY_AMP]) and float((x - y).abs().max()) <= 2e-5
        b.close()
    else:
        st = np.random.get_state()
        x = a.fetch_amp_obs_demo(301).clone()
        assert all(np.array_equal(p, q) for p, q in zip(st, np.random.get_state()) if isinstance(p, np.ndarray))          # numpy's generator is not touched
        a2 = make(True)
        assert torch.equal(x, a2.fetch_amp_obs_demo(301)) and not torch.equal(x, a.fetch_amp_obs_demo(301))
        assert x.shape == (301, 136) and torch.isfinite(x).all()
        a2.close()
    a.close()
