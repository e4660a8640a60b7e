"""The learners' episode-return meter on an MI355X (include/dyros_meter.h, csrc/dw_meter.hip): dwm_record against the g++
build of the same header bit for bit, eager against a replayed graph, and the meter inside the walk learner's loop -- eager against a torch
restatement fed by the same steps, fused and captured against the env's own episode statistics -- and the AMP learner's line."""
import ctypes as C
import importlib.util
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from isaacgymdyros_amd import game_meter as GM
from game_meter_ref import K, Synth, groups, tree_depth, unpack, work_words

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F = np.float32
U = 2.0 ** -24


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/meter_host.cpp")
    so = str(tmp_path_factory.mktemp("dwmh") / "libdwmh.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, os.path.join(ROOT, "tests", "meter_host.cpp")])
    lib = C.CDLL(so)
    P, I = C.c_void_p, C.c_int32
    lib.dwmh_record.argtypes = [I, I, I, P, P, I, P, P, P, P]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("max_size", [4, 100])
@pytest.mark.parametrize("cols", [1, 16])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_record_matches_the_host_build_bit_for_bit(host, n, cols, max_size):
    """The cases of tests/test_game_meter.py::test_host_build_matches_numpy_bit_for_bit: 40 steps, one with every env done, one with none;
    1025 envs are five workgroups, the last with one env; cur, ms and work, every word, after every launch."""
    m = GM.GameMeter(n, DEV, cols=cols, games_to_track=max_size)
    assert m.work.numel() == work_words(n, cols)
    cur, ms, work = np.zeros((cols + 1, n), F), np.zeros(K["DWM_MS_WORDS"], np.uint32), np.zeros(work_words(n, cols), np.uint32)
    syn = Synth(n, seed=1000 * n + 10 * cols + max_size)
    for t in range(40):
        rew, stacked, done = syn.step(force={10: True, 20: False}.get(t))
        if t == 30 and n > 1:
            rew[n // 2] = np.nan          # (a poisoned episode: discarded at its end, by both)
        m.record(dev(rew), dev(done), dev(stacked) if cols > 1 else None)
        host.dwmh_record(n, cols, max_size, _p(rew), _p(stacked) if cols > 1 else None, 15 if cols > 1 else 0, _p(done), _p(cur), _p(ms), _p(work))
        assert np.array_equal(m.cur.cpu().numpy().view(np.uint32), cur.view(np.uint32)), t
        got_ms, got_work = m.ms.cpu().numpy().view(np.uint32), m.work.cpu().numpy().view(np.uint32)
        assert np.array_equal(got_ms, ms), (t, np.nonzero(got_ms != ms))
        assert np.array_equal(got_work, work), (t, np.nonzero(got_work != work))
    s, want = m.summary(), unpack(ms, cols)
    assert s["games"] == want["games"] >= n and s["current_size"] == min(want["games"], max_size) and s["mean_rewards"] == want["mean"].tolist()
    assert s["window_mean_reward"] == want["sum_ret"] / want["games"] and s["window_mean_length"] == want["sum_len"] / want["games"]
    m.clear()
    assert not m.ms.cpu().numpy().any() and m.summary()["games"] == 0


def test_graph_replay_gives_the_eager_bits():
    """One record captured in a linear graph and replayed 5 times on changing inputs, against the same launches made eagerly: the ticket
    is back at zero after every launch, so a replay finds its finishing workgroup again."""
    n, cols = 1025, 16
    eager, graphed = GM.GameMeter(n, DEV, cols=cols, games_to_track=100), GM.GameMeter(n, DEV, cols=cols, games_to_track=100)
    rew, stacked, done = torch.zeros(n, device=DEV), torch.zeros(n, 15, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV)
    syn = Synth(n, seed=11, p=0.1)
    steps = [syn.step() for _ in range(7)]

    def feed(i):
        rew.copy_(dev(steps[i][0])); stacked.copy_(dev(steps[i][1])); done.copy_(dev(steps[i][2]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # (a warm-up launch on the capture stream, as a capture requires: step 0)
        feed(0)
        graphed.record(rew, done, stacked)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    feed(1)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        graphed.record(rew, done, stacked)
    torch.cuda.synchronize()
    # (the capture itself launches nothing: steps 1 .. 5 are the five replays)
    for i in range(1, 6):
        feed(i)
        g.replay()
        torch.cuda.synchronize()
        assert int(graphed.work[0]) == 0
    for i in range(0, 6):
        feed(i)
        eager.record(rew, done, stacked)
    torch.cuda.synchronize()
    for name in ("cur", "ms", "work"):
        assert torch.equal(getattr(eager, name), getattr(graphed, name)), name
    assert eager.summary()["games"] > 100


# ---------------------------------------------------------------------------------------------------- the learners
def _ppo():
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(ROOT, "examples", "ppo_consumer.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def make_env(n, episode_s, stats=False, graph=False, seed=42):
    from isaacgymdyros_amd.config import default_cfg
    from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk
    cfg = default_cfg(n, DEV)
    cfg["seed"] = seed
    cfg["env"]["episodeLength"] = episode_s          # (seconds; 0.004 s per policy step: the key ppo_player --episode-length sets)
    if stats:
        cfg["sim"]["mi355"]["episode_stats"] = True
    if graph:
        cfg["sim"]["mi355"]["device_step_counter"] = True
        cfg["sim"]["mi355"]["alias_obs"] = True
    return DyrosDynamicWalk(cfg, DEV, 0, True)


def test_walk_consumer_eager_agrees_with_a_torch_meter_fed_by_the_same_steps():
    """256 envs, horizon 16, episodes of about ten policy steps.  env.step is wrapped so that every step the loop makes also feeds a
    backend="torch" meter of the same shape.  Sizes and games agree exactly; a window mean is a convex combination of the previous mean
    and the step's, so the two meters' difference grows by at most one step's bound per update: updates * (tree depth + partial rows + 3) *
    2^-24 * scale, where scale bounds mean|x|: the number of steps made times the largest increment of the column seen."""
    ppo = _ppo()
    n, H = 256, 16
    env = make_env(n, 0.04)
    twin = GM.GameMeter(n, DEV, cols=16, games_to_track=100, backend="torch")
    seen = {"steps": 0, "updates": 0, "top": torch.zeros(17, device=DEV)}
    step = env.step

    def wrapped(a):
        o, r, d, infos = step(a)
        st = infos["stacked_rewards"]
        seen["top"] = torch.maximum(seen["top"], torch.cat([r.abs().max().view(1), st.abs().amax(dim=0), torch.ones(1, device=DEV)]))
        before = twin.summary()["games"]
        twin.record(r, d, st)
        seen["steps"] += 1
        seen["updates"] += twin.summary()["games"] > before
        return o, r, d, infos
    env.step = wrapped
    lines = []
    cfg = {"network": ppo.TRAIN_CFG["network"], "config": dict(ppo.TRAIN_CFG["config"], minibatch_size=1024, mini_epochs=1)}
    st = ppo.train(env=env, epochs=2, horizon=H, device=DEV, cfg=cfg, game_meter=True, log=lines.append)
    a, b = st[-1]["game_meter"], twin.summary()
    assert seen["steps"] == 2 * H + 1                                    # (the untimed first step is fed too)
    assert (a["current_size"], a["games"], a["discarded"]) == (b["current_size"], b["games"], b["discarded"]) and a["games"] > 100
    scale = (seen["steps"] * seen["top"]).cpu().numpy().astype(np.float64)
    tol = seen["updates"] * (tree_depth() + groups(n) + 3) * U * scale
    err = np.abs(np.asarray(a["mean_rewards"] + [a["mean_length"]]) - np.asarray(b["mean_rewards"] + [b["mean_length"]]))
    print("eager consumer: games %d, updates %d, err and tol per column: %s %s" % (a["games"], seen["updates"], err.tolist(), tol.tolist()))
    assert (err <= tol).all(), (err, tol)
    assert 5.0 <= a["mean_length"] <= 11.0 and len(a["mean_rewards"]) == 16
    assert sum("games: mean return" in x for x in lines) == 2
    env.close()


def test_walk_consumer_fused_and_captured_counts_the_episodes_the_env_counts():
    """The fused update behind a captured rollout (config 3's form), with the env's own episode statistics on: their window is one epoch,
    so the games the meter gained over an epoch are the statistics' episodes of that epoch, and the lengths' sums agree (both count every
    step of an episode, the terminating one included)."""
    ppo = _ppo()
    n, H = 512, 16
    env = make_env(n, 0.04, stats=True, graph=True)
    cfg = {"network": ppo.TRAIN_CFG["network"], "config": dict(ppo.TRAIN_CFG["config"], minibatch_size=4096, mini_epochs=1)}
    lines = []
    st = ppo.train(env=env, epochs=3, horizon=H, device=DEV, cfg=cfg, graph_rollout=True, fused_update=True, episode_stats=True, game_meter=True,
                   log=lines.append)
    for prev, s in zip(st[:-1], st[1:]):
        g0, g1, e = prev["game_meter"], s["game_meter"], s["episode_stats"]
        games = g1["games"] - g0["games"]
        assert e["records"] == H and games == e["episodes"] >= n, (games, e["episodes"])          # (every env ends an episode within 16 steps)
        len_sum = g1["window_mean_length"] * g1["games"] - g0["window_mean_length"] * g0["games"]
        print("epoch %d: games %d, mean length %.6f (meter) %.6f (episode statistics)" % (s["epoch"], games, len_sum / games, e["mean_length"]))
        assert abs(len_sum / games - e["mean_length"]) <= 1e-9 * e["mean_length"] * g1["games"]
        assert g1["discarded"] == 0 and g1["current_size"] == 100 and math.isfinite(g1["mean_reward"])
    assert sum("games: mean return" in x for x in lines) == 3
    env.close()


def run(args, timeout=600):
    p = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable] + args, cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    return p.stdout


@pytest.mark.parametrize("backend", ["hip", "torch"])
def test_amp_consumer_prints_the_meter(backend):
    cons = [os.path.join(ROOT, "examples", "amp_consumer.py"), "--synthetic", "--num_envs", "64", "--policy_backend", backend, "--epochs", "1"]
    out = run(cons + ["--game-meter"])
    m = re.search(r"^epoch 0 .*  mean_rewards (\S+)  episode length (\S+)  games (\d+)$", out, flags=re.M)
    assert m, out[-2000:]
    assert math.isfinite(float(m.group(1))) and math.isfinite(float(m.group(2))) and int(m.group(3)) >= 0
