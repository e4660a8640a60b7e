"""TocabiAMPLower's episode statistics on an MI355X (include/dyros_amp_stats.h, csrc/dw_amp_stats.hip): the HIP kernels
against the numpy restatement on synthetic buffers, the causes against the step's own reset / terminate flags in every step form, graph
replay, statistics on against off, outside resets, and both examples."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from isaacgymdyros_amd import amp_episode_stats as S
from amp_episode_stats_ref import AmpStatsRef, cause_mask, compare_raw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
K = S.K
NB = K["DWE_BODIES"]
TIME = K["DWE_C_TIME"]

# episodeLength of the witness runs.  Nobody had measured how fast this robot falls under random torques, so a first run without a limit
# (256 envs, per-env action amplitude 0 .. 1, 600 steps, reset_done() every step; tools/amp_episode_stats_time.py --lengths) gave the natural
# episode lengths, as histograms over [0, 160) in bins of 10 steps:
#   torch form, stateInit Default (1479 episodes, median 107)
#       [0, 1, 18, 39, 68, 76, 70, 52, 69, 111, 491, 419, 57, 7, 1, 0]
#   fused + rings + device draws, Default (1469 episodes, median 107)
#       [0, 1, 13, 42, 74, 68, 41, 59, 79, 102, 481, 447, 55, 6, 1, 0]
#   the same with amp_motion_device, stateInit Random on the synthetic tables (5497 episodes, median 2)
#       [3344, 120, 115, 68, 125, 211, 483, 617, 289, 95, 22, 4, 3, 1, 0, 0]
# Default starts: the limit is 100, just under the median, so that of the first generation about two in three reach it and one in three falls
# before, and two generations fit into the 200 steps.  Random motion starts are bimodal: 61 % of the starts end at their second step (the first
# one at which `progress_buf > 1` lets a fall count; a foot above 0.5 m or a thigh in the ground), and a limit at that median would make every
# step a time-limit end.  Among the starts that survive (longer than 10 steps) the median is 66: the limit there is 60.
# (The one-launch step has the fused form's starts and physics: the same limit.)
EPISODE_LENGTH = {"torch": 100, "fused": 100, "motion": 60, "one_launch": 100}
FORMS = {"torch": {}, "fused": {"amp_fused": True, "amp_hist_ring": True, "amp_device_draws": True},
         "one_launch": {"amp_fused": True, "amp_one_launch": True},
         "motion": {"amp_fused": True, "amp_hist_ring": True, "amp_device_draws": True, "amp_motion_device": True}}


def stream():
    return torch.cuda.current_stream().cuda_stream


def make_env(n, form="torch", stats=True, episode_length=None, tmp=None, seed=42):
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    cfg = default_amp_cfg(n, DEV)
    cfg["seed"] = seed
    cfg["env"]["episodeLength"] = EPISODE_LENGTH[form] if episode_length is None else episode_length
    cfg["sim"]["mi355"] = dict(FORMS[form], amp_episode_stats=stats)
    if form == "motion":
        import amp_motion_synth as SY
        cfg["env"].update({"stateInit": "Random", "motion_file": SY.write(str(tmp))})
    return TocabiAMPLower(cfg, DEV, 0, True)


def actions(n, seed=0):
    """Random actions with a per-env amplitude from 0 to 1: some envs stand until their time limit, others fall."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    amp = torch.linspace(0.0, 1.0, n, device=DEV).unsqueeze(1)
    return lambda: (torch.rand(n, 12, generator=g, device=DEV) * 2 - 1) * amp


def ref_for(env):
    return AmpStatsRef(env.num_envs, float(env.max_episode_length), float(env._termination_height), bool(env._enable_early_termination),
                       float(env.c_x[0]), float(env.c_x[1]))


def snapshot(env):
    """What dwe_record read at this step, on the host."""
    c = lambda t: t.detach().cpu().numpy().copy()          # noqa: E731
    return (c(env._root_states), c(env._contact_forces), c(env._rigid_body_pos), c(env.commands), c(env.rew_buf), c(env._reward_values),
            c(env.reset_buf), c(env.progress_buf), c(env.total_mass).reshape(-1))


# ---------------------------------------------------------------------------------------------- 1. synthetic buffers through the kernels
@pytest.mark.parametrize("n", [1, 31, 32, 33, 300])
def test_kernels_match_numpy_on_synthetic_buffers(n):
    """dwe_record / dwe_summarize called directly at the group edges of a 32-env workgroup (the tail group partly empty): every cause bit and
    the rare combinations (FLY among them), adoption, outside resets, unreset envs, non-finite rows, a window restart and restarts."""
    api = S.declare(__import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0])
    rng = np.random.default_rng(100 + n)
    ml, th, lo, hi = 60.0, 0.6, -0.5, 1.0
    ref = AmpStatsRef(n, ml, th, True, lo, hi)
    st = torch.zeros(K["DWE_ST_WORDS"], n, dtype=torch.int32, device=DEV)
    st[K["DWE_ST_N"]].fill_(-1)
    ac = torch.zeros(K["DWE_AC_WORDS"], n, dtype=torch.float32, device=DEV)
    ct = torch.zeros(K["DWE_CT_WORDS"], dtype=torch.int64, device=DEV)
    cause = torch.zeros(n, dtype=torch.uint8, device=DEV)
    out = torch.zeros(K["DWE_SUM_WORDS"], dtype=torch.float64, device=DEV)
    f = np.float32
    root, cf, rbp = np.zeros((n, 13), f), np.zeros((n, NB, 3), f), np.zeros((n, NB, 3), f)
    cmd, rew, rv = np.zeros((n, 3), f), np.zeros(n, f), np.zeros((n, 9), f)
    mass = rng.uniform(90, 110, n).astype(f)
    prog = rng.integers(0, 30, n).astype(np.int64)           # the first record adopts episodes in mid-run
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)          # noqa: E731
    seen = np.zeros(K["DWE_MASKS"], np.int64)
    for t in range(240):
        root[:] = rng.normal(0, 0.3, root.shape)
        root[:, 3:6] = rng.normal(0, 0.1, (n, 3))
        root[:, 2] = rng.uniform(0.59, 1.0, n)
        root[:, 6] = 1.0
        cf[:] = rng.normal(0, 1, cf.shape) * (rng.random((n, NB, 1)) < 0.0005) * 30
        cf[:, (8, 16), 2] = rng.uniform(0, 1600, (n, 2))
        rbp[:, (8, 16), 2] = rng.uniform(0, 0.505, (n, 2))
        cmd[:] = rng.uniform(-0.6, 1.1, (n, 3))
        rew[:] = rng.normal(0, 1, n)
        rv[:] = rng.normal(0, 1, (n, 9))
        if t % 40 == 7:
            root[rng.integers(0, n), rng.integers(0, 13)] = np.nan
        prog += 1
        reset = (cause_mask(root, cf, rbp, prog, ml, th, True) != 0).astype(np.int64)
        bufs = [d(a) for a in (root, cf, rbp, cmd, rew, rv, reset, prog, mass)]
        assert api["record"](n, *[b.data_ptr() for b in bufs], st.data_ptr(), ac.data_ptr(), ct.data_ptr(), cause.data_ptr(), ml, th, 1, lo, hi,
                             stream()) == 0
        torch.cuda.synchronize()
        want = ref.record(root, cf, rbp, cmd, rew, rv, reset, prog, mass)
        assert np.array_equal(cause.cpu().numpy(), want), t
        seen += np.bincount(want, minlength=K["DWE_MASKS"])
        if t % 60 == 0 or t == 239:
            assert np.array_equal(st.cpu().numpy()[:3], ref.si[:3]), t
            assert np.array_equal(ct.cpu().numpy(), ref.ct), t
            assert (np.abs(ac.cpu().numpy().astype(np.float64) - ref.ac) <= 1e-6 * np.maximum(np.abs(ref.ac), 1e-3)).all(), t
        done = np.nonzero(ref.si[K["DWE_ST_CLOSED"]] != 0)[0]
        done = done[rng.random(done.size) < 0.8]             # (some ended envs are reset a few steps late: unreset steps)
        prog[done] = 0
        if t % 25 == 3:
            prog[rng.integers(0, n)] = 0                     # an outside reset of a running env
        if t == 120:
            ac.zero_()
            ct[:K["DWE_CT_WINDOW"]].zero_()
            ref.reset_totals()
        if t in (90, 200):
            ids = rng.choice(n, min(5, n), replace=False)
            st[K["DWE_ST_N"]].index_fill_(0, d(ids.astype(np.int64)), -1)
            ref.restart(ids)
    assert api["summarize"](n, ac.data_ptr(), ct.data_ptr(), out.data_ptr(), stream()) == 0
    compare_raw(out.cpu().numpy(), ref.raw(), rtol=1e-6)
    s = S.fold(out.cpu().tolist(), ml, ["b%d" % g for g in range(NB)], (lo, hi))
    assert s["records"] == 119 and s["record_calls"] == 240 and s["episodes"] == sum(s["cause_masks"].values())
    if n >= 31:
        assert s["episodes"] > 0 and s["discarded"] > 0 and s["unreset_steps"] > 0
        assert all(seen[b] > 0 for b in (1, 2, 4, 8, 16)) and (seen[[m for m in range(32) if bin(m).count("1") > 1]]).sum() > 0, seen


# ---------------------------------------------------------------------------------------------- 2. / 3. the witness tests
def witness(env, steps, act, calls_before=0):
    """Steps env with reset_done() before every step; at every step the cause mask against the step's own flags, on the device; the per-step
    snapshots go through the numpy restatement.  calls_before: records the object made before this window (its count over its own life).
    -> (summary raw, restatement raw, summary)."""
    es = env.episode_stats
    ref = ref_for(env)
    ref.ct[K["DWE_CT_CALLS"]] = calls_before
    ml = float(env.max_episode_length)
    bad = torch.zeros(4, dtype=torch.int64, device=DEV)
    masks_ok = True
    for _ in range(steps):
        env.reset_done()
        _o, _r, reset, ex = env.step(act())
        c = ex["termination_cause"]
        assert c.data_ptr() == es.cause.data_ptr()
        bad[0] += ((c != 0) != (reset.view(-1) != 0)).sum()
        bad[1] += (((c & ~TIME) != 0) != (ex["terminate"].view(-1) != 0)).sum()
        bad[2] += (((c & TIME) != 0) != (env.progress_buf.float() >= ml - 1.0)).sum()
        bad[3] += (reset.view(-1) != env.reset_buf).sum()
        snap = snapshot(env)
        masks_ok &= np.array_equal(ref.record(*snap), c.cpu().numpy())
    assert bad.tolist() == [0] * 4, bad.tolist()
    assert masks_ok
    raw = es.raw()
    return raw, ref.raw(), S.fold(raw, ml, es.body_names, env.c_x)


def check_window(s, raw, want):
    compare_raw(raw, want, rtol=1e-6)
    early = sum(v for k, v in s["cause_masks"].items() if k != "time_limit")
    assert s["causes"]["time_limit"] >= 1 and early >= 1, s["cause_masks"]          # the condition on these runs
    assert s["episodes"] == sum(s["cause_masks"].values()) and "none" not in s["cause_masks"]
    assert s["discarded"] == 0 and s["unreset_steps"] == 0 and s["nonfinite_steps"] == 0
    assert all(b not in s["contact_bodies"] for b in ("L_Foot_Link", "R_Foot_Link"))
    assert all(np.isfinite(v) for v in list(s["reward_terms"].values()) + s["sole_peak_mean"] + [s["mean_return"], s["yaw_vel_error"]])


@pytest.mark.parametrize("form", ["torch", "fused", "motion", "one_launch"])
def test_causes_against_the_steps_own_flags(form, tmp_path):
    """cause != 0 <=> reset_buf, (cause & ~TIME) != 0 <=> terminate_buf, TIME <=> (float)p >= max - 1 at every step of 200, in the torch form
    (torch reset_idx), the fused form with rings and device draws (the one-launch reset_done), that with device motion starts, and the
    one-launch step with torch's draws (_reset_fused); the summary equals the restatement fed from per-step snapshots of the same run."""
    n = 256
    env = make_env(n, form, tmp=tmp_path)
    assert env._one_launch == (form == "one_launch")
    assert env._phys.episode_stats is None                   # (the cfg key does not reach the physics host)
    raw, want, s = witness(env, 200, actions(n))
    check_window(s, raw, want)
    assert s["records"] == 200 and s["sampled_steps"] == 200 * n
    env.close()


# ---------------------------------------------------------------------------------------------- 4. graph capture
def test_graph_replay_records_like_the_eager_step():
    n = 256
    env = make_env(n, "fused")
    env.reset_done()
    env.enable_graph_step(warmup=2)
    env.episode_stats.reset_totals()                         # (the warm-up and the capture's own steps are not part of the window)
    env.episode_stats.restart()
    raw, want, s = witness(env, 120, actions(n, seed=4), calls_before=2)          # (the two warm-up steps; a capture runs nothing)
    assert env._graph is not None
    check_window(s, raw, want)
    assert s["records"] == 120 and s["record_calls"] == 122
    env.close()


# ---------------------------------------------------------------------------------------------- 5. no effect on the simulation
@pytest.mark.parametrize("form", ["torch", "fused"])
def test_stats_on_and_off_give_the_same_bits(form):
    n = 256
    outs = []
    for on in (False, True):
        env = make_env(n, form, stats=on)
        assert (env.episode_stats is not None) == on
        act = actions(n, seed=2)
        h = []
        for t in range(50):
            env.reset_done()
            o, r, d, ex = env.step(act())
            h.append([o["obs"].clone(), r.clone(), d.clone(), ex["terminate"].clone(), ex["amp_obs"].clone(), env.rew_buf.clone(), env.reset_buf.clone()])
        assert ("termination_cause" in env.extras) == on
        outs.append(h)
        env.close()
    for a, b in zip(*outs):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32) if x.is_floating_point() else x, y.view(torch.int32) if y.is_floating_point() else y)


# ---------------------------------------------------------------------------------------------- 6. outside resets
@pytest.mark.parametrize("form", ["torch", "fused"])
def test_outside_resets_are_discarded_never_counted(form):
    """reset_idx() of running envs in mid-episode (torch reset_idx / _reset_fused), and buffers restored from a saved copy with restart() -- what
    a checkpoint restore of the env's buffers does; TocabiAMPLower itself has no load_state_dict()."""
    n = 256
    env = make_env(n, form, episode_length=1000)
    es = env.episode_stats
    zero = lambda: torch.zeros(n, 12, device=DEV)          # noqa: E731 (no torque: nobody falls within these steps)
    for _ in range(6):
        env.reset_done()
        env.step(zero())
    assert es.summary()["episodes"] == 0 and int(env.reset_buf.sum()) == 0
    saved = env.progress_buf.clone()
    env.reset_idx(torch.arange(0, n, 2, device=DEV))        # half of the running envs, in mid-episode
    for _ in range(3):
        env.reset_done()
        env.step(zero())
    s = es.summary()
    assert s["episodes"] == 0 and s["discarded"] == n // 2 and s["unreset_steps"] == 0
    assert torch.equal(es.st[K["DWE_ST_N"]].cpu(), torch.tensor([3, 9] * (n // 2), dtype=torch.int32))
    env.progress_buf.copy_(saved)                            # a restore: progress_buf jumps; restart() forgets the running episodes
    es.restart()
    for _ in range(2):
        env.reset_done()
        env.step(zero())
    s = es.summary()
    assert s["episodes"] == 0 and s["discarded"] == n // 2
    assert torch.equal(es.st[K["DWE_ST_N"]].cpu(), torch.full((n,), 2, dtype=torch.int32))
    es.restart(torch.tensor([5, 7], device=DEV))
    assert es.st[K["DWE_ST_N"]].cpu()[[5, 6, 7]].tolist() == [-1, 2, -1]
    env.close()


# ---------------------------------------------------------------------------------------------- 7. the examples
def run(args, timeout=600):
    p = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable] + args, cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    return p.stdout


LINE = re.compile(r"^epoch (\d+): episodes (\d+): time_limit (\S+)  non_foot_contact (\S+)  root_low (\S+)  foot_high (\S+)  tilt (\S+) \| "
                  r"contact bodies (.+) \| mean length (\S+) \| mean return (\S+) \| discarded (\d+)$", re.M)


@pytest.mark.parametrize("backend", ["hip", "torch"])
def test_examples_report_episode_stats(tmp_path, backend):
    out = str(tmp_path / "runs")
    cons = [os.path.join(ROOT, "examples", "amp_consumer.py"), "--synthetic", "--num_envs", "64", "--policy_backend", backend]
    s1 = run(cons + ["--epochs", "2", "--episode-stats", "--output_dir", out])
    lines = LINE.findall(s1)
    assert [int(m[0]) for m in lines] == [0, 1], s1[-2000:]
    for m in lines:          # (an epoch is 32 steps: it may hold no finished episode, and then the fractions are nan)
        assert int(m[10]) == 0 and (int(m[1]) == 0 or (all(0.0 <= float(x) <= 1.0 for x in m[2:7]) and np.isfinite(float(m[8])))), m
    if backend != "hip":
        return
    ck = os.path.join(out, "TocabiAMPLower", "nn", "TocabiAMPLower.pth")
    s2 = run([os.path.join(ROOT, "examples", "amp_player.py"), "--checkpoint", ck, "--synthetic", "--num_envs", "64", "--games", "64", "--report"])
    assert "av reward: " in s2 and "termination causes" in s2 and "by combination:" in s2 and "command tracking" in s2, s2[-2000:]
    m = re.search(r"^episode statistics: (\d+) episodes over (\d+) records", s2, flags=re.M)
    assert m and int(m.group(1)) >= 64
