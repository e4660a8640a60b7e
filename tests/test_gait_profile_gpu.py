"""The gait profile on an MI355X (include/dyros_gait.h, csrc/dw_gait.hip): the HIP kernels against the numpy restatement
on the synthetic buffers of tests/test_gait_profile.py, every word as an integer; then a real env, whose table is held against the step
kernel's own decisions (the foot_contact_reward it paid, the resets it made); graph replay; and the switch being off."""
import numpy as np
import pytest
import torch

from isaacgymdyros_amd import abi
from isaacgymdyros_amd import gait_profile as G
from gait_profile_ref import Synth, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, E = G.K, abi.K
W = K["DWG_W"]
STEPS, N_ENV = 300, 256


def stream():
    return torch.cuda.current_stream().cuda_stream


def api():
    return G.declare(__import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Raw:
    """Caller-owned buffers and the three entry points, called directly."""

    def __init__(self, n, bins, min_step, skip, fill=0):
        self.api, self.n, self.bins, self.min_step, self.skip = api(), n, bins, min_step, skip
        self.groups = self.api["groups"](n)
        self.part = torch.full((self.groups, bins, W), fill, dtype=torch.int64, device=DEV)
        self.ct = torch.full((K["DWG_CT_WORDS"],), fill, dtype=torch.int64, device=DEV)
        self.out = torch.full((bins * W + K["DWG_CT_WORDS"],), -1, dtype=torch.int64, device=DEV)

    def record(self, bufs):
        d = [dev(b) for b in bufs]
        assert self.api["record"](self.n, self.bins, self.min_step, int(self.skip), *[b.data_ptr() for b in d], self.part.data_ptr(),
                                  self.ct.data_ptr(), stream()) == 0, self.api["last_error"]()
        torch.cuda.synchronize()          # (d is freed after this)

    def clear(self):
        assert self.api["clear"](self.n, self.bins, self.part.data_ptr(), self.ct.data_ptr(), stream()) == 0

    def summarize(self):
        assert self.api["summarize"](self.n, self.bins, self.part.data_ptr(), self.ct.data_ptr(), self.out.data_ptr(), stream()) == 0
        o = self.out.cpu().numpy()
        return o[:self.bins * W].reshape(self.bins, W), o[self.bins * W:]


def five_records(n, bins, min_step, skip, seed):
    syn = Synth(n, seed)
    steps = [syn.step() for _ in range(5)]
    table, ct = np.zeros((bins, W), np.int64), np.zeros(K["DWG_CT_WORDS"], np.int64)
    for bufs in steps:
        record(bufs, bins, min_step, skip, table, ct)
    return steps, table, ct


# ---------------------------------------------------------------------------------------------- synthetic buffers through the kernels
@pytest.mark.parametrize("bins,min_step,skip", [(12, 0, False), (72, 5, False), (144, 5, True)])
@pytest.mark.parametrize("n", [1, 33, 257, 1000])
def test_kernels_match_numpy_as_integers(n, bins, min_step, skip):
    """n = 1 and 33: a partial wave; 257: four whole workgroups and one env in a fifth; 1000: sixteen workgroups, the last with 40 envs."""
    steps, table, ct = five_records(n, bins, min_step, skip, 100 * n + bins)
    r = Raw(n, bins, min_step, skip)
    assert r.groups == (n + K["DWG_GROUP"] - 1) // K["DWG_GROUP"]
    for bufs in steps:
        r.record(bufs)
    got, gct = r.summarize()
    assert np.array_equal(gct, ct), (gct, ct)
    assert np.array_equal(got, table), np.argwhere(got != table)[:10]
    assert int(ct.sum()) == 5 * n and int(got[:, 0].sum()) == int(ct[0])
    assert np.array_equal(r.part.cpu().numpy().sum(axis=0), table)          # (out is the sum of the workgroups' partial tables)
    if n >= 257:
        assert ct[K["DWG_CT_RECORDED"]] > 0 and ct[K["DWG_CT_SKIPPED_TERMINAL"]] > 0 and (ct[K["DWG_CT_SKIPPED_FILTER"]] > 0) == (min_step > 0)


def test_a_non_finite_word_is_discarded_on_the_gpu_as_on_the_host():
    n, bins = 257, 72
    table, ct = np.zeros((bins, W), np.int64), np.zeros(K["DWG_CT_WORDS"], np.int64)
    r = Raw(n, bins, 0, False)
    for i, span in enumerate(("sole_r", "dof_pos", "target_qpos", "action_torque", "paid", "total_mass")):
        bufs = Synth(n, 40 + i, nan_span=span, unread_nan=True).step()
        record(bufs, bins, 0, False, table, ct)
        r.record(bufs)
    got, gct = r.summarize()
    assert np.array_equal(gct, ct) and np.array_equal(got, table) and ct[K["DWG_CT_DISCARDED"]] > 6 * 60


def test_clear_then_the_same_records_give_the_same_table():
    n, bins = 257, 72
    steps, table, ct = five_records(n, bins, 0, False, 9)
    r = Raw(n, bins, 0, False, fill=-12345)          # (buffers that were never zeroed: dwg_clear is what starts a window)
    r.clear()
    assert not r.part.any() and not r.ct.any()
    for rounds in range(2):
        for bufs in steps:
            r.record(bufs)
        got, gct = r.summarize()
        assert np.array_equal(gct, ct) and np.array_equal(got, table), rounds
        r.clear()
    got, gct = r.summarize()
    assert not got.any() and not gct.any()


# ---------------------------------------------------------------------------------------------- a real env
def make_env(n, profile=None, **mi):
    from isaacgymdyros_amd.config import default_cfg
    from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk
    cfg = default_cfg(n, DEV)
    cfg["seed"] = 42
    cfg["env"]["episodeLength"] = 2.0          # (seconds; 0.004 s per policy step: the time limit is past the run's 300 steps)
    cfg["sim"]["mi355"]["device_step_counter"] = True
    cfg["sim"]["mi355"]["alias_obs"] = True
    cfg["sim"]["mi355"].update(mi)
    if profile is not None:
        cfg["sim"]["mi355"]["gait_profile"] = profile
    return DyrosDynamicWalk(cfg, DEV, 0, True)


def action_list(n, steps, seed=0):
    """Random actions with a per-env amplitude: some envs stand through the run, others fall (as tests/test_run_trace_gpu.py)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    amp = torch.tensor([0.0, 0.05, 0.3, 1.0], device=DEV)[torch.arange(n, device=DEV) % 4].view(1, n, 1)
    return ((torch.rand(steps, n, 13, generator=g, device=DEV) * 2 - 1) * amp).contiguous()


@pytest.fixture(scope="module")
def eager():
    """The 300 eager steps every test below shares: the summary, and per step the step kernel's own reset flags, mocap index and
    foot_contact_reward column."""
    env = make_env(N_ENV, {"bins": 72})
    acts = action_list(N_ENV, STEPS)
    a = torch.zeros(N_ENV, 13, device=DEV)
    snaps = []
    for i in range(STEPS):
        a.copy_(acts[i])
        env.step(a)
        snaps.append(torch.stack([env._buf["reset_buf"].to(torch.float64), abi.es_view(env._buf["env_state"], "mocap_data_idx").to(torch.float64).reshape(-1),
                                  env._buf["stacked_rewards"][:, K["DWG_PAID_COLUMN"]].to(torch.float64)]))
    table, ct = env.gait_profile.raw()
    s = env.gait_profile.summary()
    env.close()
    return {"table": table, "ct": ct, "summary": s, "snaps": torch.stack(snaps).cpu().numpy(), "acts": acts}


def test_the_table_agrees_with_the_step_kernels_own_decisions(eager):
    table, ct, snaps = eager["table"], eager["ct"], eager["snaps"]
    reset, idx, paid = snaps[:, 0] != 0, snaps[:, 1].astype(np.int64), snaps[:, 2]
    total = N_ENV * STEPS
    count = table[:, K["DWG_R_COUNT"]]
    print("recorded %d of %d env-steps; counters %s; per window count / paid / predicted: %s" % (
        count.sum(), total, ct.tolist(), {n: (w["count"], w["paid_fraction"], w["paid_predicted_fraction"]) for n, w in eager["summary"]["windows"].items()}))
    assert idx.min() >= 0 and idx.max() <= 3598
    want_paid = np.zeros(72, np.int64)
    np.add.at(want_paid, idx[~reset] // 50, (paid[~reset] > 0).astype(np.int64))
    assert np.array_equal(table[:, K["DWG_R_PAID"]], want_paid)
    assert np.array_equal(table[:, K["DWG_R_PREDICTED"]], table[:, K["DWG_R_PAID"]]), np.argwhere(table[:, K["DWG_R_PREDICTED"]] != table[:, K["DWG_R_PAID"]])
    assert int(count.sum()) + int(ct[K["DWG_CT_SKIPPED_TERMINAL"]] + ct[K["DWG_CT_SKIPPED_FILTER"]] + ct[K["DWG_CT_DISCARDED"]]) == total
    assert int(ct[K["DWG_CT_RECORDED"]]) == int(count.sum())
    assert int(ct[K["DWG_CT_SKIPPED_TERMINAL"]]) == int(reset.sum()) > 0
    # not vacuous
    assert int(count.sum()) >= 0.9 * total
    w = eager["summary"]["windows"]
    assert w["DSP"]["count"] > 0 and (w["RSSP"]["count"] > 0 or w["LSSP"]["count"] > 0)
    assert w["DSP"]["paid_fraction"] * w["DSP"]["count"] > 0
    # the per-bin counts are the host's from the snapshots
    want_count = np.zeros(72, np.int64)
    np.add.at(want_count, idx[~reset] // 50, 1)
    assert np.array_equal(count, want_count) and ct[K["DWG_CT_DISCARDED"]] == 0


def test_summary_of_the_real_run_is_consistent(eager, tmp_path):
    s = eager["summary"]
    assert np.array_equal(s["table"], eager["table"]) and s["bins"] == 72 and s["recorded"] == int(eager["ct"][0])
    seen = s["count"] > 0
    assert np.isfinite(s["fz"][seen]).all() and (s["fz_std"][seen] >= 0).all() and (s["root_z"][seen] > 0.3).all()
    assert (s["expected_fz"][seen] >= 0).all() and 0 < s["duty_factor"][0] <= 1 and 0 < s["duty_factor"][1] <= 1
    G.write_npz(str(tmp_path / "g.npz"), s)
    assert np.array_equal(np.load(str(tmp_path / "g.npz"))["table"], eager["table"])
    assert len(open(G.write_txt(str(tmp_path), s)).read().splitlines()) == 73


def test_graph_replay_gives_the_eager_summary_bit_for_bit(eager):
    """Step and record captured in one graph and replayed, on the same actions: the 64-bit sums do not depend on the order of the adds."""
    env = make_env(N_ENV, {"bins": 72})
    acts = eager["acts"]
    a = torch.zeros(N_ENV, 13, device=DEV)
    a.copy_(acts[0])
    env.step(a)                            # (the first step is eager on both sides)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        env.step(a)                        # (a linear chain: the step, the counter, the record)
    for i in range(1, STEPS):
        a.copy_(acts[i])
        g.replay()
    torch.cuda.synchronize()
    table, ct = env.gait_profile.raw()
    env.close()
    assert np.array_equal(ct, eager["ct"]) and np.array_equal(table, eager["table"])


def test_off_by_default_and_no_launch_is_added(monkeypatch):
    calls = []
    monkeypatch.setattr(G.GaitProfile, "record", lambda self: calls.append(1))
    env = make_env(64)
    assert env.gait_profile is None and "gait_profile" not in env.cfg["sim"]["mi355"]
    for _ in range(3):
        env.step(torch.zeros(64, 13, device=DEV))
    env.close()
    assert calls == []          # (step() reaches the recorder only through `if self.gait_profile is not None`)
    env = make_env(64, profile=False)
    assert env.gait_profile is None
    env.close()
    env = make_env(64, profile=True)
    assert isinstance(env.gait_profile, G.GaitProfile) and env.gait_profile.bins == 72
    for _ in range(3):
        env.step(torch.zeros(64, 13, device=DEV))
    env.close()
    assert calls == [1, 1, 1]


def test_profile_on_and_off_give_the_same_simulation(eager):
    """The recorder only reads the step's buffers: observations, rewards and resets are the same bits with the profile on, off, and on
    beside the other two recorders."""
    outs = []
    for profile, mi in ((None, {}), ({"bins": 144, "min_episode_step": 3, "skip_pushes": True}, {}),
                        (True, {"episode_stats": True, "run_trace": {"env_ids": 8, "depth": 4, "hold": "never"}})):
        env = make_env(N_ENV, profile, **mi)
        a, h = torch.zeros(N_ENV, 13, device=DEV), []
        for i in range(40):
            a.copy_(eager["acts"][i])
            o, r, d, _ex = env.step(a)
            h.append(torch.cat([o["obs"].reshape(-1).view(torch.int32), r.reshape(-1).view(torch.int32), d.reshape(-1).to(torch.int32)]))
        outs.append(torch.stack(h).cpu())
        env.close()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and bool(outs[0][:, -N_ENV:].any())


# ---------------------------------------------------------------------------------------------- the learner
def test_consumer_logs_one_window_per_epoch():
    """The fused update behind a captured rollout with the profile on: every epoch is one window of the epoch's env-steps."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                               "examples", "ppo_consumer.py"))
    ppo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ppo)
    n, H = 512, 16
    cfg = {"network": ppo.TRAIN_CFG["network"], "config": dict(ppo.TRAIN_CFG["config"], minibatch_size=4096, mini_epochs=1)}
    lines = []
    st = ppo.train(num_envs=n, epochs=3, horizon=H, device=DEV, cfg=cfg, graph_rollout=True, fused_update=True, gait_profile={"bins": 36},
                   log=lines.append)
    for e, s in enumerate(st):
        g = s["gait_profile"]
        steps = g["recorded"] + g["skipped_terminal"] + g["skipped_filter"] + g["discarded"]
        # (the first window also holds the steps the loop makes before its first epoch: the untimed first step and the capture's warm-up)
        assert g["bins"] == 36 and steps % n == 0 and (steps == n * H if e > 0 else n * H <= steps <= n * (H + 8)), (e, steps)
        assert g["recorded"] == int(g["count"].sum()) == sum(w["count"] for w in g["windows"].values()) > 0
    assert st[0]["gait_profile"]["windows"]["DSP"]["count"] > 0          # (every env starts its first episode in double support)
    assert sum("gait: DSP paid" in x for x in lines) == 3
    plain = ppo.train(num_envs=n, epochs=1, horizon=H, device=DEV, cfg=cfg, graph_rollout=True, fused_update=True, log=lambda _s: None)
    assert "gait_profile" not in plain[0]


# ---------------------------------------------------------------------------------------------- the command lines
def test_consumer_flag_and_player_report(tmp_path):
    """examples/ppo_consumer.py --gait-profile logs its line per epoch; examples/ppo_player.py --gait-report prints the three-window table and
    --gait-dir writes the two files."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(args):
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable] + args, cwd=root, capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
        return p.stdout
    out = str(tmp_path / "runs")
    s1 = run([os.path.join(root, "examples", "ppo_consumer.py"), "--fused", "--num-envs", "1024", "--horizon", "32", "--epochs", "1", "--output-dir", out,
              "--gait-profile"])
    assert len(re.findall(r"^epoch 1: gait: DSP paid \S+ \|F err\| \S+ \S+  RSSP paid .*LSSP paid .*\(\d+ env-steps\)$", s1, flags=re.M)) == 1, s1[-2000:]
    gdir = str(tmp_path / "gait")
    s2 = run([os.path.join(root, "examples", "ppo_player.py"), "--checkpoint", os.path.join(out, "DyrosDynamicWalk", "nn", "DyrosDynamicWalk.pth"),
              "--num-envs", "64", "--games", "64", "--gait-report", "--gait-dir", gdir, "--gait-bins", "24"])
    m = re.search(r"^gait profile: (\d+) env-steps in 24 bins \((\d+) terminal", s2, flags=re.M)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) >= 64, s2[-2000:]
    assert all(re.search(r"^  %s +\d+ " % w, s2, flags=re.M) for w in G.WINDOWS), s2[-2000:]
    z = np.load(os.path.join(gdir, "gait_profile.npz"))
    assert z["table"].shape == (24, W) and int(z["recorded"]) == int(m.group(1)) == int(z["table"][:, 0].sum())
    assert len(G.read_txt(os.path.join(gdir, "gait_profile.txt"))["bin"]) == 24
