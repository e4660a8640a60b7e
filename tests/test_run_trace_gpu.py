"""The run trace on an MI355X (include/dyros_trace.h, csrc/dw_trace.hip): the HIP kernels against the numpy restatement on
the synthetic buffers of tests/test_run_trace.py, then a real env: the rings against per-step clones of the env's own attributes, the hold
at a fall, explicit restarts, trace on vs off, graph replay, and the player."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from isaacgymdyros_amd import abi
from isaacgymdyros_amd import run_trace as T
from run_trace_ref import Synth, TraceRef, non_foot_max

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
K, E = T.K, abi.K
N_SYN, ML_SYN = 37, 9.0


def stream():
    return torch.cuda.current_stream().cuda_stream


def make_env(n, episode_s, trace=None, stats=False, step_dev=False, seed=42, **mi):
    from isaacgymdyros_amd.config import default_cfg
    from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk
    cfg = default_cfg(n, DEV)
    cfg["seed"] = seed
    cfg["env"]["episodeLength"] = episode_s          # (seconds; 0.004 s per policy step)
    cfg["sim"]["mi355"]["episode_stats"] = stats
    cfg["sim"]["mi355"]["device_step_counter"] = step_dev
    cfg["sim"]["mi355"].update(mi)
    if trace is not None:
        cfg["sim"]["mi355"]["run_trace"] = trace
    return DyrosDynamicWalk(cfg, DEV, 0, True)


def actions(n, seed=0):
    """Random actions with a per-env amplitude: some envs stand until their time limit, others fall (as tests/test_episode_stats_gpu.py)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    amp = torch.tensor([0.0, 0.05, 0.3, 1.0], device=DEV)[torch.arange(n, device=DEV) % 4].unsqueeze(1)
    return lambda: (torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * amp


# ---------------------------------------------------------------------------------------------- 1. synthetic buffers through the kernels
@pytest.mark.parametrize("hold", ["never", "fall", "reset"])
@pytest.mark.parametrize("depth", [1, 4, 7])
@pytest.mark.parametrize("k", [1, 3, 4, 5, 37])
def test_kernels_match_numpy_on_synthetic_buffers(k, depth, hold):
    """The cases of tests/test_run_trace.py::test_record_matches_numpy_bit_for_bit: k = 5 and 37 put slots past one workgroup, k = 1 and 3
    leave a partial one."""
    api = T.declare(__import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0])
    n = N_SYN
    env_ids = np.random.default_rng(k).permutation(n)[:k].tolist()
    ref = TraceRef(n, env_ids, depth, hold, ML_SYN)
    syn = Synth(n, ML_SYN, 100 * k + depth)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)          # noqa: E731
    ring = torch.zeros(k, depth, K["DWT_ROW_WORDS"], dtype=torch.int32, device=DEV)
    ss = torch.zeros(K["DWT_SS_WORDS"], k, dtype=torch.int32, device=DEV)
    slot_env, env_slot = d(ref.slot_env), d(ref.env_slot)

    def arm(ids=None):
        t_ids = None if ids is None else d(np.asarray(ids, np.int32))
        assert api["arm"](n, k, None if t_ids is None else t_ids.data_ptr(), 0 if t_ids is None else t_ids.numel(), d(syn.count).data_ptr(),
                          env_slot.data_ptr(), ss.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        ref.arm(syn.count, ids)

    def same():
        assert np.array_equal(ss.cpu().numpy().view(np.uint32), ref.ss)
        assert np.array_equal(ring.cpu().numpy().view(np.uint32), ref.ring)
    arm()
    same()
    for t in range(3 * depth + 2):
        bufs = syn.step()
        dev = [d(b) for b in bufs]
        assert api["record"](n, k, depth, T.HOLD[hold], slot_env.data_ptr(), *[b.data_ptr() for b in dev], ML_SYN, ss.data_ptr(), ring.data_ptr(),
                             stream()) == 0
        torch.cuda.synchronize()
        ref.record(*bufs)
        same()
        if hold != "never" and t == 2 * depth:
            arm(ref.slot_env[::2])
            same()
    slots = list(range(k)) + [k + 3, -1]          # (a slot id out of range gives zero rows)
    out = torch.full((len(slots), depth, K["DWT_ROW_WORDS"]), -1, dtype=torch.int32, device=DEV)
    rows = torch.full((len(slots),), -7, dtype=torch.int32, device=DEV)
    assert api["gather"](k, depth, d(np.asarray(slots, np.int32)).data_ptr(), len(slots), ss.data_ptr(), ring.data_ptr(), out.data_ptr(),
                         rows.data_ptr(), stream()) == 0
    want, want_rows = ref.gather(slots)
    assert np.array_equal(rows.cpu().numpy(), want_rows) and np.array_equal(out.cpu().numpy().view(np.uint32), want)


def test_non_foot_maximum_ties_and_zero_row_on_the_gpu():
    api = T.declare(__import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0])
    n, k = N_SYN, 4
    ref = TraceRef(n, [0, 1, 2, 3], 2, "never", ML_SYN)
    bufs = list(Synth(n, ML_SYN, 0).step(fall_p=0.0))
    cf = np.zeros((n, E["DW_NUM_BODIES"], 3), np.float32)
    cf[0, 30], cf[0, 11], cf[0, 8], cf[0, 16] = (0.0, 3.0, 4.0), (3.0, 4.0, 0.0), (0.0, 0.0, 900.0), (0.0, 0.0, 800.0)
    cf[2, 37], cf[3, 8] = (0.0, 0.0, -2.0), (1.0, 2.0, 3.0)
    bufs[2] = cf
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)          # noqa: E731
    ring = torch.zeros(k, 2, K["DWT_ROW_WORDS"], dtype=torch.int32, device=DEV)
    ss = torch.zeros(K["DWT_SS_WORDS"], k, dtype=torch.int32, device=DEV)
    dev = [d(b) for b in bufs]
    assert api["record"](n, k, 2, 0, d(ref.slot_env).data_ptr(), *[b.data_ptr() for b in dev], ML_SYN, ss.data_ptr(), ring.data_ptr(), stream()) == 0
    ref.record(*bufs)
    got = ring.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, ref.ring)
    out = T.decode(got)
    assert out["non_foot_max"][:, 0].tolist() == [5.0, 0.0, 2.0, 0.0] and out["non_foot_body"][:, 0].tolist() == [11.0, 0.0, 37.0, 0.0]


# ---------------------------------------------------------------------------------------------- a real env next to the restatement
CLONED = ("root_states", "dof_state", "contact_forces", "env_state", "rew_buf", "stacked_rewards", "reset_buf", "timeout_buf")


class Shadow:
    """Steps a traced env and, after every step, clones the env's own buffers and attributes; the numpy restatement records from the clones."""

    def __init__(self, env, seed):
        self.env, self.tr = env, env.run_trace
        self.act = actions(env.num_envs, seed)
        self.ref = TraceRef(env.num_envs, self.tr.env_ids, self.tr.depth, self.tr.hold, float(env.max_episode_length))
        self.ref.arm(env.progress_buf.cpu().numpy())
        self.steps = []          # per step: the clones (numpy), progress_buf before the step, held() after it

    def step(self):
        env = self.env
        p0 = env.progress_buf.clone()
        env.step(self.act())
        c = {k: env._buf[k].clone() for k in CLONED}
        attr = {k: getattr(env, k).clone() for k in ("dof_pos", "dof_vel", "qpos_noise", "target_data_qpos", "action_torque", "target_data_force",
                                                      "target_vel", "magnitude", "phase", "time", "pert_on", "perturb_start", "nan_resets")}
        attr["actions"] = abi.es_view(env._buf["env_state"], "actions").clone()
        held = self.tr.held().clone()
        c = {k: v.cpu().numpy() for k, v in c.items()}
        c["dof_state"] = c["dof_state"].reshape(env.num_envs, 33, 2)
        self.ref.record(*[c[k] for k in CLONED])
        self.steps.append(dict(c, p0=p0.cpu().numpy(), held=held.cpu().numpy(), **{k: v.cpu().numpy() for k, v in attr.items()}))

    def same(self):
        torch.cuda.synchronize()
        assert np.array_equal(self.tr.ss.cpu().numpy().view(np.uint32), self.ref.ss)
        assert np.array_equal(self.tr.ring.cpu().numpy().view(np.uint32), self.ref.ring)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check_row(r, i, j, st, e, ml):
    """Row j of read()'s entry i against the clones `st` of the step that wrote it, for env e: channel by channel, bitwise."""
    for name, src in (("root_states", st["root_states"][e]), ("dof_pos", st["dof_pos"][e]), ("dof_vel", st["dof_vel"][e]),
                      ("qpos_noise", st["qpos_noise"][e]), ("target_data_qpos", st["target_data_qpos"][e]), ("actions", st["actions"][e]),
                      ("action_torque", st["action_torque"][e]), ("foot_forces", st["contact_forces"][e][[8, 16]]),
                      ("target_data_force", st["target_data_force"][e]), ("target_vel", st["target_vel"][e]), ("magnitude", st["magnitude"][e]),
                      ("phase", st["phase"][e]), ("time", st["time"][e, 0]), ("rew_buf", st["rew_buf"][e]),
                      ("stacked_rewards", st["stacked_rewards"][e]), ("nan_resets", st["nan_resets"][e])):
        assert np.array_equal(bits(r[name][i, j]), bits(np.asarray(src))), (name, i, j)
    v, g = non_foot_max(st["contact_forces"][e][None])
    assert bits(r["non_foot_max"][i, j]) == bits(v)[0] and r["non_foot_body"][i, j] == float(g[0])
    assert r["epi_step"][i, j] == st["p0"][e] + 1
    f = r["flags"]
    assert f["reset"][i, j] == (st["reset_buf"][e] != 0) and f["timeout"][i, j] == (st["timeout_buf"][e] != 0)
    assert f["time_limit"][i, j] == (np.float32(st["p0"][e] + 1) >= np.float32(ml) - np.float32(1.0))
    assert f["pert_on"][i, j] == (st["pert_on"][e] != 0) and f["perturb_start"][i, j] == (st["perturb_start"][e, 0] != 0)


def test_real_env_rings_equal_per_step_clones():
    n, depth, steps = 256, 16, 120
    env = make_env(n, 0.2, trace={"env_ids": n, "depth": depth, "hold": "never"})          # 50-step episodes: time limits occur
    sh = Shadow(env, seed=5)
    for _ in range(steps):
        sh.step()
    sh.same()
    r = env.run_trace.read()
    ml = float(env.max_episode_length)
    assert r["rows"].tolist() == [depth] * n and r["cursor"].tolist() == [steps] * n and not r["held"].any()
    assert (r["seen"] == np.arange(steps - depth + 1, steps + 1)[None, :]).all() and (r["pad"] == 0).all()
    for j in range(depth):
        st = sh.steps[steps - depth + j]
        for e in range(n):
            check_row(r, e, j, st, e, ml)
    resets = np.stack([s["reset_buf"] != 0 for s in sh.steps])
    limits = np.stack([np.float32(s["p0"] + 1) >= np.float32(ml) - 1 for s in sh.steps])
    assert (resets & limits).any() and (resets & ~limits).any()          # both kinds of end occurred
    assert r["falls"].tolist() == (resets & ~limits).sum(0).tolist()
    env.close()


def test_real_env_hold_at_a_fall():
    n, depth = 256, 32
    env = make_env(n, 0.4, trace={"env_ids": n, "depth": depth, "hold": "fall"})          # 100-step episodes: the standing envs reach the limit
    tr = env.run_trace
    sh = Shadow(env, seed=6)
    ml = float(env.max_episode_length)
    while len(sh.steps) < 400:
        sh.step()
        if len(sh.steps) % 20 == 0 and int(sh.steps[-1]["held"].sum()) >= n // 4:
            break
    sh.same()
    held = np.nonzero(sh.steps[-1]["held"])[0]
    assert len(held) >= n // 4, (len(held), len(sh.steps))
    # no slot is held by a time limit, and time limits did occur on slots that were recording
    seen_limit = 0
    for t, st in enumerate(sh.steps):
        before = sh.steps[t - 1]["held"] if t else np.zeros(n, bool)
        limit = (st["reset_buf"] != 0) & (np.float32(st["p0"] + 1) >= np.float32(ml) - 1) & ~before
        seen_limit += int(limit.sum())
        assert not st["held"][limit].any()
    assert seen_limit > 0
    r = tr.read(held)
    f = r["flags"]
    last = r["rows"] - 1
    idx = np.arange(len(held))
    assert f["reset"][idx, last].all() and not f["time_limit"][idx, last].any()
    assert (r["rows"] == np.minimum(r["cursor"], depth)).all() and r["held"].all() and (r["falls"] >= 1).all()
    for i, e in enumerate(held):          # every row against the clones of the step that wrote it (row's seen = that step's number)
        for j in range(int(r["rows"][i])):
            check_row(r, i, j, sh.steps[int(r["seen"][i, j]) - 1], e, ml)
    # ten further steps change nothing but `seen`
    ring0, ss0 = tr.ring.clone(), tr.ss.clone()
    for _ in range(10):
        sh.step()
    sh.same()
    hs = torch.from_numpy(held).to(DEV)
    assert torch.equal(tr.ring[hs], ring0[hs])
    for w in ("CURSOR", "HELD", "N", "FALLS"):
        assert torch.equal(tr.ss[K["DWT_SS_" + w]][hs], ss0[K["DWT_SS_" + w]][hs])
    assert torch.equal(tr.ss[K["DWT_SS_SEEN"]][hs], ss0[K["DWT_SS_SEEN"]][hs] + 10)
    # arm() makes the slots record again
    sub = held[: len(held) // 2]
    tr.arm(torch.from_numpy(sub).to(DEV))
    sh.ref.arm(env.progress_buf.cpu().numpy(), sub)
    sh.step()
    sh.same()
    cur = tr.ss[K["DWT_SS_CURSOR"]].cpu().numpy()
    assert (cur[sub] == 1).all() and np.array_equal(cur[held[len(sub):]], ss0[K["DWT_SS_CURSOR"]].cpu().numpy()[held[len(sub):]])
    ep = tr.episodes(int(sub[0]))
    assert len(ep) == 1 and len(ep[0]["seen"]) == 1
    env.close()


def test_explicit_restarts_arm_the_slots_they_touch():
    n = 256
    ids = list(range(0, 128, 2)) + [200, 201]
    env = make_env(n, 0.6, trace={"env_ids": ids, "depth": 8, "hold": "reset"})
    tr = env.run_trace
    act = actions(n, seed=1)
    for _ in range(10):
        env.step(act())
    saved = env.state_dict()
    ss0 = tr.ss.cpu().numpy().copy()
    touched = torch.arange(0, 64, device=DEV)          # traced: the even ones
    env.reset_idx(touched)
    torch.cuda.synchronize()
    ss1, prog = tr.ss.cpu().numpy(), env.progress_buf.cpu().numpy()
    hit = np.array([e < 64 for e in ids])
    for w in ("CURSOR", "HELD", "SEEN", "FALLS"):
        assert not ss1[K["DWT_SS_" + w], hit].any()
        assert np.array_equal(ss1[K["DWT_SS_" + w], ~hit], ss0[K["DWT_SS_" + w], ~hit])
    assert np.array_equal(ss1[K["DWT_SS_N"], hit], prog[np.array(ids)[hit]]) and np.array_equal(ss1[K["DWT_SS_N"], ~hit], ss0[K["DWT_SS_N"], ~hit])
    assert (ss0[K["DWT_SS_CURSOR"]] > 0).all()
    for _ in range(5):
        env.step(act())
    env.load_state_dict(saved)
    torch.cuda.synchronize()
    ss2 = tr.ss.cpu().numpy()
    for w in ("CURSOR", "HELD", "SEEN", "FALLS"):
        assert not ss2[K["DWT_SS_" + w]].any()
    assert np.array_equal(ss2[K["DWT_SS_N"]], env.progress_buf.cpu().numpy()[ids])
    env.step(act())
    r = tr.read([200, 0])
    assert r["rows"].tolist() == [1, 1] and r["epi_step"][:, 0].tolist() == (saved["progress_buf"][[200, 0]] + 1).tolist()
    # retarget: other envs, every slot cleared
    tr.retarget(list(range(n - len(ids), n)))
    env.step(act())
    r = tr.read()
    assert r["env_ids"].tolist() == list(range(n - len(ids), n)) and r["rows"].tolist() == [1] * len(ids)
    assert np.array_equal(bits(r["root_states"][:, 0]), bits(env.root_states.cpu().numpy()[n - len(ids):]))
    with pytest.raises(ValueError, match="not traced"):
        tr.read([0])
    env.close()


# ---------------------------------------------------------------------------------------------- no effect on the simulation
def test_trace_on_off_and_beside_the_stats_give_the_same_bits():
    n = 256
    outs = []
    for trace, stats in ((None, False), ({"env_ids": 64, "depth": 16, "hold": "fall"}, False), ({"env_ids": n, "depth": 4, "hold": "never"}, True)):
        env = make_env(n, 0.2, trace=trace, stats=stats)
        assert (env.run_trace is not None) == (trace is not None)
        act = actions(n, seed=2)
        h = []
        for _ in range(50):
            o, r, d, _ex = env.step(act())
            h.append([o["obs"].clone(), r.clone(), d.clone()])
        torch.cuda.synchronize()
        outs.append(h)
        env.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            for x, y in zip(a, b):
                assert torch.equal(x.view(torch.int32) if x.is_floating_point() else x, y.view(torch.int32) if y.is_floating_point() else y)


# ---------------------------------------------------------------------------------------------- graph capture
def test_graph_replay_gives_the_eager_ring_bit_for_bit():
    n, k = 512, 20
    got = []
    for captured in (False, True):
        env = make_env(n, 0.2, trace={"env_ids": list(range(0, 2 * 70, 2)), "depth": 32, "hold": "fall"}, step_dev=True, alias_obs=True)
        a = (torch.rand(n, 13, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV) * 2 - 1).contiguous()
        env.step(a)                            # (untimed first step on both sides)
        torch.cuda.synchronize()
        if captured:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                env.step(a)                    # (a linear chain: the step, the counter, the record)
            for _ in range(k):
                g.replay()
        else:
            for _ in range(k):
                env.step(a)
        torch.cuda.synchronize()
        got.append((env.run_trace.ring.cpu(), env.run_trace.ss.cpu()))
        env.close()
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert int(got[0][1][K["DWT_SS_SEEN"]].min()) == k + 1 and int(got[0][1][K["DWT_SS_CURSOR"]].min()) > 0


# ---------------------------------------------------------------------------------------------- the player
def test_player_writes_the_falls(tmp_path):
    import importlib.util
    from isaacgymdyros_amd import ppo_checkpoint as PK
    from isaacgymdyros_amd import ppo_update as U
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(ROOT, "examples", "ppo_consumer.py"))
    ppo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ppo)
    torch.manual_seed(3)
    net = ppo.DyrosActorCritic(U.IN, U.ACT, ppo.TRAIN_CFG["network"]).to(DEV)          # an untrained policy: it falls
    c = ppo.TRAIN_CFG["config"]
    ck = PK.save(str(tmp_path / "p.pth"), net, epoch=0, opt_actor=torch.optim.Adam(net.actor_parameters(), lr=c["learning_rate"]),
                 opt_critic=torch.optim.Adam(net.critic_parameters(), lr=c["critic_lr"]))
    out = tmp_path / "traces"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_player.py"), "--checkpoint", ck, "--num-envs", "64", "--games", "32",
                        "--max-steps", "600", "--episode-length", "0.8", "--stochastic", "--trace-dir", str(out), "--trace-envs", "16",
                        "--trace-depth", "24", "--trace-hold", "fall"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted(f for f in os.listdir(out) if f.startswith("fall_env") and f.endswith(".npz"))
    assert files and "run trace: %d files written" % len(files) in r.stdout, r.stdout[-2000:]
    for name in files:
        z = np.load(out / name)
        rows = len(z["seen"])
        assert 1 <= rows <= 24 and z["root_states"].shape == (rows, 13) and z["dof_pos"].shape == (rows, 33) and z["foot_forces"].shape == (rows, 2, 3)
        assert z["flag_reset"][-1] and not z["flag_time_limit"][-1]          # the ring ends with the fall
        assert z["held"] and int(z["env_id"]) < 16
        # the decoding round-trips: the named flags are the raw bits', and the rows are consecutive steps of one episode
        for flag, bit in T.FLAGS.items():
            assert np.array_equal(z["flag_" + flag], (z["flags"] & bit) != 0)
        assert (np.diff(z["seen"]) == 1).all()
        assert np.array_equal(z["epi_step"][1:], np.where(z["flag_reset"][:-1], 1, z["epi_step"][:-1] + 1))


# ---------------------------------------------------------------------------------------------- drains
def test_drain_reads_held_slots_and_arms_them_again():
    n = 256
    env = make_env(n, 0.4, trace={"env_ids": n, "depth": 16, "hold": "fall"})
    tr = env.run_trace
    act = actions(n, seed=7)
    assert tr.drain(8) == []                                     # nothing held yet
    for _ in range(400):
        env.step(act())
        if int(tr.held().sum()) >= 12:
            break
    held0 = tr.held().cpu().numpy()
    assert held0.sum() >= 12
    ring0 = tr.ring.cpu().numpy().view(np.uint32)
    falls = tr.drain(8)
    assert len(falls) == 8 and len({f["env_id"] for f in falls}) == 8
    held1, cur1 = tr.held().cpu().numpy(), tr.ss[K["DWT_SS_CURSOR"]].cpu().numpy()
    for f in falls:
        e = f["env_id"]                                          # (all envs traced in order: slot == env)
        assert held0[e] and f["held"] and not held1[e] and cur1[e] == 0
        assert f["flags"]["reset"][-1] and not f["flags"]["time_limit"][-1] and 1 <= len(f["seen"]) <= 16
        assert np.array_equal(bits(f["root_states"][-1]), ring0[e, (f["cursor"] - 1) % 16, K["DWT_CH_ROOT"]:K["DWT_CH_ROOT"] + 13])
    assert held1.sum() == held0.sum() - 8 and not (held1 & ~held0).any()
    rest = tr.drain()                                            # all that is left
    assert len(rest) == held0.sum() - 8 and not tr.held().any()
    env.close()


def test_consumer_writes_falls_per_epoch(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(ROOT, "examples", "ppo_consumer.py"))
    ppo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ppo)
    stats = ppo.train(num_envs=2048, epochs=2, graph_rollout=True, fused_update=True, trace_falls=str(tmp_path / "falls"), log=lambda _s: None)
    files = [f for s in stats for f in s["trace_falls"]]
    assert all(len(s["trace_falls"]) <= ppo.TRACE_DRAIN for s in stats) and files and len(set(files)) == len(files)
    for path in files:
        z = np.load(path)
        assert z["flag_reset"][-1] and not z["flag_time_limit"][-1] and int(z["env_id"]) < 64 and z["dof_pos"].shape[1] == 33
    plain = ppo.train(num_envs=2048, epochs=1, graph_rollout=True, fused_update=True, log=lambda _s: None)
    assert "trace_falls" not in plain[0]
