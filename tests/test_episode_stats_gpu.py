"""Episode statistics on an MI355X (include/dyros_stats.h, csrc/dw_stats.hip): the HIP kernels against the numpy
restatement, the causes against the step kernel's own flags, the NaN guard, restarts, stats on vs off, graph replay, the metrics of a real run,
and both examples."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from isaacgymdyros_amd import abi
from isaacgymdyros_amd import episode_stats as S
from episode_stats_ref import StatsRef, compare_raw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
K, E = S.K, abi.K
NB, ESW = E["DW_NUM_BODIES"], E["DW_ES_WORDS"]
SENT = -123.0


def stream():
    return torch.cuda.current_stream().cuda_stream


def make_env(n, episode_s=0.6, stats=True, wave_build=0, terrain=False, step_dev=False, seed=42, **mi):
    from isaacgymdyros_amd.config import default_cfg, with_terrain
    from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk
    cfg = default_cfg(n, DEV)
    cfg["seed"] = seed
    cfg["env"]["deathCost"] = SENT
    cfg["env"]["episodeLength"] = episode_s
    cfg["sim"]["mi355"]["episode_stats"] = stats
    cfg["sim"]["mi355"]["debug_wave_build"] = wave_build
    cfg["sim"]["mi355"]["device_step_counter"] = step_dev
    cfg["sim"]["mi355"].update(mi)
    if terrain:
        cfg = with_terrain(cfg, mesh_type="trimesh", curriculum=True)
    return DyrosDynamicWalk(cfg, DEV, 0, True)


def actions(n, seed=0):
    """Random actions with a per-env amplitude: some envs stand until their time limit, others fall."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    amp = torch.tensor([0.0, 0.05, 0.3, 1.0], device=DEV)[torch.arange(n, device=DEV) % 4].unsqueeze(1)
    return lambda: (torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * amp


# ---------------------------------------------------------------------------------------------- 1. synthetic buffers through the kernels
@pytest.mark.parametrize("n", [1, 31, 32, 33, 37, 300])
def test_kernels_match_numpy_on_synthetic_buffers(n):
    api = S.declare(__import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0])
    rng = np.random.default_rng(n)
    ml, dtp = 60.0, 0.004
    ref = StatsRef(n, ml, dtp)
    st = torch.zeros(K["DWS_ST_WORDS"], n, dtype=torch.int32, device=DEV)
    ac = torch.zeros(K["DWS_AC_WORDS"], n, dtype=torch.float32, device=DEV)
    ct = torch.zeros(K["DWS_CT_WORDS"], dtype=torch.int64, device=DEV)
    cause = torch.zeros(n, dtype=torch.uint8, device=DEV)
    out = torch.zeros(K["DWS_SUM_WORDS"], dtype=torch.float64, device=DEV)
    root = np.zeros((n, 13), np.float32)
    cf = np.zeros((n, NB, 3), np.float32)
    es = np.zeros((n, ESW), np.float32)
    esi = es.view(np.int32)
    mass = rng.uniform(90, 110, n).astype(np.float32)
    prog = np.zeros(n, np.int64)
    es[:, E["DW_ES_TARGET_VEL"]] = rng.uniform(0, 0.8, n)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)          # noqa: E731

    def restart(ids=None):
        t_ids = None if ids is None else d(np.asarray(ids, np.int32))
        assert api["restart"](n, None if t_ids is None else t_ids.data_ptr(), 0 if t_ids is None else t_ids.numel(), d(root).data_ptr(),
                              d(es).data_ptr(), d(prog).data_ptr(), st.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        ref.restart(root, es, prog, ids)
    restart()
    for t in range(300):
        root[:] = rng.normal(0, 1, root.shape)
        cf[:] = rng.normal(0, 1, cf.shape) * (rng.random((n, NB, 1)) < 0.02) * 30
        cf[:, 8, 2] = rng.uniform(0, 1600, n)
        cf[:, 16, 2] = rng.uniform(0, 1600, n)
        es[:, E["DW_ES_TARGET_FORCE"]:E["DW_ES_TARGET_FORCE"] + 2] = rng.normal(0, 5, (n, 2))
        es[:, E["DW_ES_ACTION_TORQUE"]:E["DW_ES_ACTION_TORQUE"] + 24] = rng.normal(0, 20, (n, 24))
        es[:, E["DW_ES_LAST_RETURN"]] = rng.normal(0, 10, n)
        esi[:, E["DW_ES_PERT_ON"]] = rng.random(n) < 0.1
        esi[:, E["DW_ES_NAN_RESETS"]] += rng.random(n) < 0.01
        esi[0, E["DW_ES_PERT_START"]] = int(t >= 120)
        reset = ((rng.random(n) < 0.05) | (ref.si[K["DWS_ST_N"]] + 1 >= 59)).astype(np.int64)
        es[reset != 0, E["DW_ES_TARGET_VEL"]] = rng.uniform(0, 0.8, int(reset.sum()))
        assert api["record"](n, d(root).data_ptr(), d(cf).data_ptr(), d(es).data_ptr(), d(reset).data_ptr(), d(mass).data_ptr(), st.data_ptr(),
                             ac.data_ptr(), ct.data_ptr(), cause.data_ptr(), ml, dtp, stream()) == 0
        torch.cuda.synchronize()
        want = ref.record(root, cf, es, reset, mass)
        assert np.array_equal(cause.cpu().numpy(), want), t
        if t % 50 == 0 or t == 299:
            assert np.array_equal(st.cpu().numpy().view(np.uint32), ref.st), t
            assert np.array_equal(ac.cpu().numpy(), ref.ac), t
            assert np.array_equal(ct.cpu().numpy(), ref.ct), t
        if t == 150:
            ac.zero_()
            ct[:K["DWS_CT_WINDOW"]].zero_()
            ref.reset_totals()
        if t in (90, 200):
            ids = rng.choice(n, min(5, n), replace=False)
            prog[ids] = rng.integers(0, 50, 5)[:len(ids)]
            restart(ids)
    assert api["summarize"](n, ac.data_ptr(), ct.data_ptr(), out.data_ptr(), stream()) == 0
    compare_raw(out.cpu().numpy(), ref.raw(), rtol=1e-12)
    s = S.fold(out.cpu().tolist(), n, ml, ["b%d" % g for g in range(NB)])
    assert s["perturb_start_at_record"] == 120 and sum(s["causes"].values()) == s["episodes"] > 0


# ---------------------------------------------------------------------------------------------- 2. the witness test
@pytest.mark.parametrize("n,wave_build,terrain", [(4096, 3, False), (8192, 1, False), (16384, 2, False), (4096, 0, True)],
                         ids=["hex-4096", "oct1-8192", "oct2-16384", "heightfield-4096"])
def test_causes_against_the_step_kernels_own_flags(n, wave_build, terrain):
    """deathCost is a sentinel: the step kernel writes it into all 14 stacked reward terms iff its collision flag was set, and into rew_buf iff
    collision or orientation fired.  So every step's causes are checked against the kernel's own decisions -- which also pins that an in-step
    reset leaves the env's contact_forces row as the last substep wrote it."""
    env = make_env(n, wave_build=wave_build, terrain=terrain)
    es = env.episode_stats
    act = actions(n)
    ml = float(env.max_episode_length)
    ep0 = env.episodes_finished.clone()
    len_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    bad = torch.zeros(5, dtype=torch.int64, device=DEV)
    seen = torch.zeros(5, dtype=torch.int64, device=DEV)
    env.reset()
    for _ in range(300):
        p = env.progress_buf.clone()
        nan0 = env.nan_resets.reshape(-1).clone()
        _o, rew, reset, ex = env.step(act())
        c = ex["termination_cause"]
        assert c.data_ptr() == es.cause.data_ptr()
        r = reset.view(-1) != 0
        coll = (ex["stacked_rewards"][:, :14] == SENT).all(1)
        tl = (p + 1).float() >= ml - 1.0
        bad[0] += ((c != 0) != r).sum()
        bad[1] += ((c == 2) != coll).sum()
        bad[2] += ((c == 3) & ((rew.view(-1) != SENT) | coll)).sum()
        bad[3] += (((c == 1) != (tl & ~coll)) & (c != 4)).sum()
        bad[4] += ((c == 4) != (env.nan_resets.reshape(-1) > nan0)).sum()
        seen += torch.bincount(c.long(), minlength=5)
        len_sum += torch.where(r, env.epi_len_log.reshape(-1).double(), 0.0).sum()
    s = es.summary()
    assert bad.tolist() == [0] * 5, bad.tolist()
    assert int((env.episodes_finished - ep0).sum()) == s["episodes"]
    assert s["mean_length"] == pytest.approx(float(len_sum) / s["episodes"], rel=1e-12)
    assert seen[1:4].min() > 0, seen.tolist()
    assert sum(s["causes"].values()) == s["episodes"]
    assert s["contact_bodies"] and all(b not in s["contact_bodies"] for b in ("L_Foot_Link", "R_Foot_Link"))
    env.close()


# ---------------------------------------------------------------------------------------------- 3. the NaN guard
def test_non_finite_root_state_is_its_own_cause():
    env = make_env(256)
    act = actions(256)
    for _ in range(5):
        env.step(act())
    nan0 = env.nan_resets.clone()
    env.root_states[[3, 100, 200], 3] = float("nan")
    _o, _r, reset, ex = env.step(act())
    c = ex["termination_cause"].cpu()
    assert [int(c[i]) for i in (3, 100, 200)] == [4, 4, 4]
    d = (env.nan_resets - nan0).view(-1).cpu()
    assert [int(d[i]) for i in (3, 100, 200)] == [1, 1, 1] and int(d.sum()) == 3
    assert es_causes(env)["non_finite"] == 3
    env.close()


def es_causes(env):
    return env.episode_stats.summary()["causes"]


# ---------------------------------------------------------------------------------------------- 4. restarts
def test_reset_idx_and_load_state_dict_discard_running_episodes():
    n = 512
    env = make_env(n, episode_s=0.2)          # 50 steps
    es = env.episode_stats
    act = actions(n, seed=1)
    for _ in range(20):
        env.step(act())
    saved = env.state_dict()
    es.reset_totals()
    ep0 = int(env.episodes_finished.sum())
    env.reset_idx(torch.arange(0, n, 2, device=DEV))
    torch.cuda.synchronize()
    st = es.st.cpu()
    assert torch.equal(st[K["DWS_ST_N"]].long(), env.progress_buf.cpu()), "counters restart from progress_buf"
    assert int(st[K["DWS_ST_NR"], 0::2].abs().sum()) == 0
    assert es.summary()["episodes"] == 0 and int(env.episodes_finished.sum()) == ep0, "the discarded episodes are not counted"
    for _ in range(15):
        env.step(act())
    env.load_state_dict(saved)
    torch.cuda.synchronize()
    assert torch.equal(es.st.cpu()[K["DWS_ST_N"]].long(), env.progress_buf.cpu())
    es.reset_totals()
    ep0 = env.episodes_finished.clone()
    for _ in range(60):                       # past every env's time limit: the count agrees with the kernel's after both restarts
        p = env.progress_buf.clone()
        _o, _r, reset, ex = env.step(act())
        tl = (p + 1).float() >= float(env.max_episode_length) - 1.0
        coll = (ex["stacked_rewards"][:, :14] == SENT).all(1)
        c = ex["termination_cause"]
        assert int((((c == 1) != (tl & ~coll)) & (c != 4)).sum()) == 0
    assert es.summary()["episodes"] == int((env.episodes_finished - ep0).sum())
    env.close()


# ---------------------------------------------------------------------------------------------- 5. no effect on the simulation
def test_stats_on_and_off_give_the_same_bits():
    n = 1024
    outs = []
    for on in (False, True):
        env = make_env(n, stats=on)
        act = actions(n, seed=2)
        h = []
        for t in range(200):
            o, r, d, ex = env.step(act())
            if t % 20 == 19 or t == 199:
                h.append([o["obs"].clone(), r.clone(), d.clone(), ex["time_outs"].clone(), ex["stacked_rewards"].clone()])
        torch.cuda.synchronize()
        h.append([env._buf["env_state"].clone(), env.root_states.clone(), env._buf["dof_state"].clone(), env.contact_forces.clone()])
        assert ("termination_cause" in env.extras) == on
        outs.append(h)
        env.close()
    for a, b in zip(*outs):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.uint8) if x.is_floating_point() else x, y.view(torch.uint8) if y.is_floating_point() else y)


# ---------------------------------------------------------------------------------------------- 6. graph capture
def test_graph_replay_gives_the_eager_summary_bit_for_bit():
    n, k = 2048, 120
    raws = []
    for captured in (False, True):
        env = make_env(n, step_dev=True, alias_obs=True)
        a = (torch.rand(n, 13, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV) * 2 - 1).contiguous()
        env.step(a)                            # (untimed first step on both sides)
        torch.cuda.synchronize()
        if captured:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                env.step(a)
            for _ in range(k):
                g.replay()
        else:
            for _ in range(k):
                env.step(a)
        torch.cuda.synchronize()
        raws.append(env.episode_stats.raw())
        env.close()
    assert raws[0] == raws[1]
    assert raws[0][K["DWS_CT_RECORDS"]] == k + 1 and raws[0][K["DWS_CT_EPISODES"]] > 0


# ---------------------------------------------------------------------------------------------- 7. the metrics of a real run
def test_metrics_match_a_restatement_from_per_step_snapshots():
    n = 512
    env = make_env(n, episode_s=0.6)
    es = env.episode_stats
    act = actions(n, seed=3)
    snap = lambda: (env.root_states.cpu().numpy(), env.contact_forces.cpu().numpy(), env._buf["env_state"].cpu().numpy())          # noqa: E731
    root, cf, est = snap()
    ref = StatsRef(n, float(env.max_episode_length), float(env.dt_policy))
    ref.restart(root, est, env.progress_buf.cpu().numpy())
    mass = env._buf["total_mass"].cpu().numpy().reshape(n)
    a0 = E["DW_ES_ACTION_TORQUE"]
    # the torque difference on its own, from consecutive action_torque snapshots: per env the max |tau_t - tau_t-1| over the records of an
    # episode that have an earlier record of the same episode, summed over ended episodes
    prev, have, run_max, dtm_sum = np.zeros((n, 12), np.float32), np.zeros(n, bool), np.zeros(n, np.float32), 0.0
    pre_is_tau = True
    for _ in range(300):
        _o, _r, reset, ex = env.step(act())
        root, cf, est = snap()
        rs = reset.cpu().numpy() != 0
        got = ex["termination_cause"].cpu().numpy()
        want = ref.record(root, cf, est, rs, mass)
        assert np.array_equal(got, want)
        tau = est[:, a0:a0 + 12]
        pre_is_tau &= np.array_equal(est[:, a0 + 12:a0 + 24], tau)          # (the step's late update: why tau_pre cannot serve)
        run_max = np.where(have, np.maximum(run_max, np.abs(tau - prev).max(1)), run_max)
        dtm_sum += float(run_max[rs].astype(np.float64).sum())
        prev = np.where(rs[:, None], 0.0, tau).astype(np.float32)
        have = ~rs
        run_max = np.where(rs, 0.0, run_max).astype(np.float32)
    s = es.summary()
    compare_raw(es.raw(), ref.raw(), rtol=1e-5)
    assert s["episodes"] > 0 and all(np.isfinite(v) for v in s["force_tracking_error"] + s["sole_peak_mean"])
    assert pre_is_tau
    assert s["torque_diff_max_mean"] > 1.0
    assert s["torque_diff_max_mean"] == pytest.approx(dtm_sum / s["episodes"], rel=1e-5)
    env.close()


# ---------------------------------------------------------------------------------------------- 8. / 9. the examples
def _consumer():
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(ROOT, "examples", "ppo_consumer.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_consumer_reports_episode_stats_per_epoch(tmp_path):
    ppo = _consumer()
    lines = []
    stats = ppo.train(num_envs=2048, epochs=2, graph_rollout=True, fused_update=True, episode_stats=True, log=lines.append,
                      output_dir=str(tmp_path))
    for s in stats:
        e = s["episode_stats"]
        assert sum(e["causes"].values()) == e["episodes"]
        assert e["records"] == int(ppo.TRAIN_CFG["config"]["horizon_length"])          # (the window is the epoch's rollout)
        flat = [e["mean_length"], e["mean_return"], e["torque_mean"]] + e["sole_peak_mean"] + e["force_tracking_error"]
        assert all(np.isfinite(v) for v in flat if e["episodes"])
    assert sum("contact bodies" in ln for ln in lines) == 2
    plain = ppo.train(num_envs=2048, epochs=1, graph_rollout=True, fused_update=True, log=lines.append)
    assert "episode_stats" not in plain[0]
    ck = os.path.join(str(tmp_path), "DyrosDynamicWalk", "nn", "DyrosDynamicWalk.pth")
    assert os.path.exists(ck)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_player.py"), "--checkpoint", ck, "--report", "--nominal",
                        "--num-envs", "64", "--games", "64", "--max-steps", "400", "--episode-length", "0.4"], capture_output=True, text=True,
                       timeout=600)          # (100-step episodes: every game ends by its time limit at the latest)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "nominal environment" in r.stdout and "termination causes" in r.stdout and "perturbation gate" in r.stdout, r.stdout[-2000:]
