"""The learners' episode-return meter without a GPU (include/dyros_meter.h, isaacgymdyros_amd/csrc/dw_meter.h): the
arithmetic -- compiled by g++ from the header the HIP kernel includes (tests/meter_host.cpp) -- against hand-worked answers, against the
numpy float32 restatement of tests/game_meter_ref.py bit for bit, and against a float64 restatement within a derived bound; the
best-checkpoint policy against a table; the derived prototypes; GameMeter's argument checks; and the walk learner's loop with the meter on."""
import ctypes as C
import importlib.util
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from isaacgymdyros_amd import build
from isaacgymdyros_amd import game_meter as GM
from game_meter_ref import GROUP, HEAD, K, MeterRef, Synth, groups, step64, tree_depth, unpack, work_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -24          # the unit roundoff of float32


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
    lib.dwmh_clear.argtypes = [P, P]
    lib.dwmh_work_words.argtypes = [I, I]
    lib.dwmh_work_words.restype = C.c_int64
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Host:
    """The g++ build's buffers and calls."""

    def __init__(self, lib, n, cols, max_size):
        self.lib, self.n, self.cols, self.max_size = lib, n, cols, max_size
        assert lib.dwmh_work_words(n, cols) == work_words(n, cols)
        self.cur = np.zeros((cols + 1, n), F)
        self.ms = np.zeros(K["DWM_MS_WORDS"], np.uint32)
        self.work = np.zeros(work_words(n, cols), np.uint32)

    def record(self, rew, stacked, done):
        rew, done = np.ascontiguousarray(rew, F), np.ascontiguousarray(done, np.int64)
        st = None if self.cols == 1 else np.ascontiguousarray(stacked, F)
        self.lib.dwmh_record(self.n, self.cols, self.max_size, _p(rew), None if st is None else _p(st), 0 if st is None else st.shape[1], _p(done),
                             _p(self.cur), _p(self.ms), _p(self.work))

    def clear(self):
        self.lib.dwmh_clear(_p(self.ms), _p(self.work))

    def state(self):
        return unpack(self.ms, self.cols)


def test_hand_worked_window_answers(host):
    """max_size = 4, eight envs, one column: every expected value below is worked by hand from include/dyros_meter.h's rule and is exact in
    float32 (the sums are small integers and halves, the divisors 1, 3, 4 and 6 divide them)."""
    h = Host(host, 8, 1, 4)
    # k = 6: returns 1..6 -> new_mean 3.5; size = min(6, 4) = 4, old = min(4 - 4, 0) = 0 -> mean 3.5; every length 1
    def S(x):
        d = x.state()
        return dict(d, mean=d["mean"].tolist())
    h.record([1, 2, 3, 4, 5, 6, 7, 8], None, [1, 1, 1, 1, 1, 1, 0, 0])
    assert S(h) == {"current_size": 4, "mean": [3.5], "mean_len": 1.0, "games": 6, "discarded": 0, "sum_ret": 21.0, "sum_len": 6.0}
    assert h.cur.tolist() == [[0, 0, 0, 0, 0, 0, 7, 8], [0, 0, 0, 0, 0, 0, 1, 1]]
    # k = 1: env 6 ends with 7 + 1 = 8 after 2 steps; size 1, old = min(4 - 1, 4) = 3 -> (3.5 * 3 + 8 * 1) / 4 = 4.625, (1 * 3 + 2) / 4 = 1.25
    h.record([1] * 8, None, [0, 0, 0, 0, 0, 0, 5, 0])
    assert S(h) == {"current_size": 4, "mean": [4.625], "mean_len": 1.25, "games": 7, "discarded": 0, "sum_ret": 29.0, "sum_len": 8.0}
    # k = 0: nothing of ms moves, bit for bit; the running episodes go on
    before = h.ms.copy()
    h.record([0.5] * 8, None, [0] * 8)
    assert np.array_equal(h.ms, before)
    assert h.cur.tolist() == [[1.5] * 6 + [0.5, 9.5], [2] * 6 + [1, 3]]
    # k = 3 from current_size 4: envs 0, 6, 7 end with 1.5 + 2.5 = 4, 0.5 + 1.5 = 2, 9.5 + 2.5 = 12 after 3, 2, 4 steps -> new_mean 6 and 3;
    # size 3, old = min(4 - 3, 4) = 1 -> (4.625 * 1 + 6 * 3) / 4 = 5.65625, (1.25 * 1 + 3 * 3) / 4 = 2.5625
    h.record([2.5, 0, 0, 0, 0, 0, 1.5, 2.5], None, [1, 0, 0, 0, 0, 0, 1, 1])
    assert S(h) == {"current_size": 4, "mean": [5.65625], "mean_len": 2.5625, "games": 10, "discarded": 0, "sum_ret": 47.0, "sum_len": 17.0}
    assert h.cur.tolist() == [[0, 1.5, 1.5, 1.5, 1.5, 1.5, 0, 0], [0, 3, 3, 3, 3, 3, 0, 0]]
    assert h.work[0] == 0          # the ticket
    # a window that is not full: max_size 4, k = 1 twice from empty -> sizes 1, 2
    g = Host(host, 8, 1, 4)
    g.record([3] * 8, None, [0, 0, 1, 0, 0, 0, 0, 0])
    assert (S(g)["current_size"], S(g)["mean"]) == (1, [3.0])
    g.record([1] * 8, None, [0, 0, 0, 1, 0, 0, 0, 0])          # env 3 ends with 4: (3 * 1 + 4 * 1) / 2
    assert (S(g)["current_size"], S(g)["mean"], S(g)["mean_len"]) == (2, [3.5], 1.5)
    g.clear()
    assert not g.ms.any() and g.cur[0, 0] == 4.0          # (clear() leaves the running episodes)


@pytest.mark.parametrize("max_size", [4, 100])
@pytest.mark.parametrize("cols", [1, 16])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_host_build_matches_numpy_bit_for_bit(host, n, cols, max_size):
    """40 steps with a done probability of 0.02, one step where every env is done and one where none is: cur, ms and work, every word."""
    h, ref, syn = Host(host, n, cols, max_size), MeterRef(n, cols, max_size), Synth(n, seed=1000 * n + 10 * cols + max_size)
    games = 0
    for t in range(40):
        rew, stacked, done = syn.step(force={10: True, 20: False}.get(t))
        h.record(rew, stacked, done)
        games += ref.record(rew, stacked, done)
        assert np.array_equal(h.cur.view(np.uint32), ref.cur.view(np.uint32)), t
        assert np.array_equal(h.ms, ref.ms), (t, np.nonzero(h.ms != ref.ms))
        assert np.array_equal(h.work, ref.work), (t, np.nonzero(h.work != ref.work))
    s = h.state()
    assert s["games"] == games >= n and s["discarded"] == 0 and s["current_size"] == min(games, max_size)
    if cols == 16:          # (mixed-sign term columns)
        assert (s["mean"] > 0).any() and (s["mean"] < 0).any()


@pytest.mark.parametrize("max_size", [100, 1000])
@pytest.mark.parametrize("cols", [1, 16])
@pytest.mark.parametrize("n", [257, 1025])
def test_host_build_against_float64_step_by_step(host, n, cols, max_size):
    """Every step's means against a float64 restatement that starts from the meter's own previous means and size, so that the difference
    is ONE step's rounding.  Allowed: (tree depth + number of partial rows + 3) * 2^-24 * mean|x| over the done envs, per column.

    Derivation, from the order include/dyros_meter.h documents, to first order in u = 2^-24, for one column with terms x_i, i in D, |D| = k,
    m = mean|x| = sum|x_i| / k, G partial rows, M = |previous mean|, w = old / (old + size), result r = (M' * old + new_mean * size) / (old + size):
      * a term reaches its workgroup's partial sum through at most 6 butterfly additions and 3 wavefront additions (tree depth d = 9) and
        the total through at most G more (row 0 is added to +0, which is exact, so G - 1; G is kept): |total - sum x| <= (d + G) u sum|x|.
      * new_mean = total / k is one rounding, new_mean * size one, mean * old one, their sum one, the last division one.
      * so |error| <= u [ (d + G + 2) (1 - w) m  +  w M  +  2 |r| ]  and  |r| <= (1 - w) m + w M:
            |error| <= u [ (d + G + 4) (1 - w) m + 3 w M ].
      * old = 0 (w = 0, always the case once k >= max_size): mean * 0 is exact and so is the sum with it: (d + G + 3) u m.  This is the bound.
      * old > 0: the expression is at most (d + G + 3) u m exactly when 3 w M <= ((d + G + 4) w - 1) m: the previous mean must not dwarf
        what this step averages, and the window must not be nearly empty.  The test's data are made for that -- a done probability of 0.25
        gives k of about N / 4, so from the second update on old is 0 or a good part of the window, and a stationary reward keeps the
        previous mean near the finished episodes' mean |x| -- and the premise is asserted on the inputs at every step and column.
    The lengths (column C) are bounded alike."""
    h, syn = Host(host, n, cols, max_size), Synth(n, seed=7 * n + cols + max_size, p=0.25)
    factor = tree_depth() + groups(n) + 3
    checked = 0
    for t in range(30):
        rew, stacked, done = syn.step()
        cur0, s0 = h.cur.copy(), h.state()
        h.record(rew, stacked, done)
        s1 = h.state()
        prev = np.append(s0["mean"], s0["mean_len"]).astype(np.float64)
        k, want, m = step64(cur0, rew, stacked, done, cols, max_size, prev, s0["current_size"])
        got = np.append(s1["mean"], s1["mean_len"]).astype(np.float64)
        if k == 0:
            assert np.array_equal(got, prev)
            continue
        size = min(k, max_size)
        old = min(max_size - size, s0["current_size"])
        w = old / (old + size)
        assert old == 0 or (3 * w * np.abs(prev) <= ((factor + 1) * w - 1) * m).all(), (t, old, size, prev, m)          # the derivation's premise
        err = np.abs(got - want)
        print("n %d cols %d max_size %d step %d: k %d old %d  max err / (u mean|x|) = %.3f of %d allowed" % (n, cols, max_size, t, k, old, (err / (U * m)).max(), factor))
        assert (err <= factor * U * m).all(), (t, err / (U * m), factor)
        checked += 1
    assert checked >= 25


def test_non_finite_returns_are_discarded_and_counted(host):
    n = 300
    h, ref = Host(host, n, 2, 100), MeterRef(n, 2, 100)
    rng = np.random.default_rng(3)
    for t in range(6):
        rew = rng.normal(1.0, 1.0, n).astype(F)
        stacked = rng.normal(0.0, 1.0, (n, 15)).astype(F)
        done = np.zeros(n, np.int64)
        if t == 1:
            rew[7], stacked[260, 0], stacked[9, 1] = np.nan, np.inf, np.nan          # (column 1 of `stacked` is no column of a meter of two)
        if t == 3:
            done[[7, 260, 9, 11, 299]] = 1
        h.record(rew, stacked, done)
        ref.record(rew, stacked, done)
        assert np.array_equal(h.ms, ref.ms) and np.array_equal(h.cur.view(np.uint32), ref.cur.view(np.uint32)) and np.array_equal(h.work, ref.work)
        if t == 2:
            assert np.isnan(h.cur[0, 7]) and np.isinf(h.cur[1, 260]) and np.isfinite(h.cur[:, 9]).all()
        if t == 3:          # every done env is cleared, the poisoned ones too
            assert not h.cur[:, [7, 260, 9, 11, 299]].any() and np.isfinite(h.cur).all()
    s = h.state()
    assert (s["games"], s["discarded"], s["current_size"]) == (3, 2, 3)                      # envs 9, 11, 299 averaged; 7 and 260 discarded
    assert np.isfinite(s["mean"]).all() and math.isfinite(s["mean_len"]) and s["mean_len"] == 4.0 and math.isfinite(s["sum_ret"])
    assert np.isfinite(h.cur).all() and (h.cur[2, [7, 260, 9, 11, 299]] == 2.0).all()
    # a step in which every finished episode is discarded moves no mean
    before = h.ms.copy()
    rew = np.ones(n, F); rew[5] = -np.inf
    done = np.zeros(n, np.int64); done[5] = 1
    h.record(rew, np.zeros((n, 15), F), done)
    after = h.state()
    assert after["discarded"] == 3 and after["games"] == 3
    changed = np.nonzero(h.ms != before)[0].tolist()
    assert changed == [K["DWM_MS_DISCARDED"]]


def test_layout_constants():
    assert K["DWM_ABI_VERSION"] == 1 and K["DWM_COLS_MAX"] == 16 and GROUP == 256 and GM.COLS_MAX == 16
    assert K["DWM_MS_MEAN"] + 16 == K["DWM_MS_MEAN_LEN"] < K["DWM_MS_GAMES"] and K["DWM_MS_SUM_LEN"] + 2 == K["DWM_MS_WORDS"]
    assert all(K[k] % 2 == 0 for k in ("DWM_MS_GAMES", "DWM_MS_DISCARDED", "DWM_MS_SUM_RET", "DWM_MS_SUM_LEN"))
    assert work_words(16384, 16) == HEAD + 64 * 19 and work_words(1, 1) == HEAD + 4


# (epoch, mean) -> files, should_exit; save_frequency 2, save_best_after 3, score_to_win 50, from rl_games' -100500
TABLE = [
    (1, 5.0, [], False),                                               # above the best, before save_best_after, not a save_frequency epoch: nothing
    (2, 5.0, [], False),                                               # a save_frequency epoch, but above the best (-100500): no last_ file either
    (3, 4.0, ["X"], False),                                            # epoch == save_best_after: the best moves to 4
    (4, 4.0, ["last_X_ep_4_rew_4.0"], False),                          # equal to the best: not a new best; a save_frequency epoch
    (5, 3.5, [], False),                                               # below the best, no save_frequency epoch
    (6, 4.5, ["X"], False),                                            # a new best on a save_frequency epoch: the best file only
    (8, 1.25, ["last_X_ep_8_rew_1.25"], False),
    (9, 50.0, ["X"], False),                                           # equal to score_to_win: not past it
    (10, 50.5, ["X", "X_ep_10_rew_50.5"], True),                       # past score_to_win
]


def test_best_checkpoints_follow_the_reference_policy():
    b = GM.BestCheckpoints("X", 2, 3, 50, GM.LAST_MEAN_REWARDS)
    assert b.last_mean_rewards == -100500
    best = -100500
    for epoch, mean, files, done in TABLE:
        assert b.after_epoch(epoch, mean) == (files, done), (epoch, mean)
        if "X" in files:
            best = mean
        assert b.last_mean_rewards == best
    assert b.final(11, 50.5) == "last_Xep11rew50.5"
    # save_frequency 0: no last_ files; a resumed best holds
    r = GM.BestCheckpoints("X", 0, 0, 50, last_mean_rewards=7.0)
    assert r.after_epoch(4, 7.0) == ([], False) and r.after_epoch(5, 6.0) == ([], False) and r.after_epoch(6, 7.5) == (["X"], False)
    # the mean is printed as the reference's numpy float32 prints
    assert GM.BestCheckpoints("X", 1, 0, 50, 100.0).after_epoch(3, float(np.float32(1.1))) == (["last_X_ep_3_rew_1.1"], False)
    assert "torch" not in GM.BestCheckpoints.after_epoch.__code__.co_names + GM.BestCheckpoints.__init__.__code__.co_names


def test_ctypes_prototypes_match_the_header():
    import test_cbind as TC
    TC.test_ctypes_prototypes_match_the_header("dyros_meter.h", "dwm_", "game_meter", C.CDLL(build.build()))
    assert sorted(GM.EXPORTS) == ["abi_version", "clear", "last_error", "record", "work_words"]


def test_library_refuses_bad_shapes():
    lib = C.CDLL(build.build())
    api = GM.declare(lib)
    assert api["work_words"](16384, 16) == work_words(16384, 16) and api["work_words"](1, 1) == work_words(1, 1)
    assert api["work_words"](0, 1) == -1 and b"num_envs" in api["last_error"]()
    assert api["work_words"](8, 17) == -1 and b"cols" in api["last_error"]()
    one = (C.c_float * 8)()          # (every call below is refused before anything is launched)
    for args, what in (((0, 1, 4, one, None, 0, one, one, one, one, None), b"num_envs"), ((8, 0, 4, one, None, 0, one, one, one, one, None), b"cols"),
                       ((8, 1, 0, one, None, 0, one, one, one, one, None), b"max_size"), ((8, 2, 4, one, None, 15, one, one, one, one, None), b"stacked"),
                       ((8, 3, 4, one, one, 1, one, one, one, one, None), b"stacked_stride"), ((8, 1, 4, None, None, 0, one, one, one, one, None), b"missing")):
        assert api["record"](*args) == -1 and what in api["last_error"](), (args[:3], api["last_error"]())
    assert api["clear"](None, one, None) == -1


def test_game_meter_checks_its_arguments():
    with pytest.raises(ValueError, match="needs a GPU"):
        GM.GameMeter(8, "cpu")
    for kw, what in ((dict(cols=0), "cols"), (dict(cols=17), "cols"), (dict(games_to_track=0), "games_to_track"), (dict(backend="numpy"), "backend")):
        with pytest.raises(ValueError, match=what):
            GM.GameMeter(8, "cpu", **dict(dict(backend="torch"), **kw))
    with pytest.raises(ValueError, match="num_envs"):
        GM.GameMeter(0, "cpu", backend="torch")
    m = GM.GameMeter(8, "cpu", cols=3, backend="torch")
    rew, done, st = torch.ones(8), torch.zeros(8, dtype=torch.int64), torch.zeros(8, 15)
    for args, what in (((rew.double(), done, st), "rew: dtype"), ((torch.ones(7), done, st), "rew: 7 elements"), ((rew, torch.zeros(9, dtype=torch.int64), st), "done: 9"),
                       ((rew, done.int(), st), "done: dtype"), ((rew, done, None), "stacked"), ((rew, done, torch.zeros(8, 1)), "stacked: shape"),
                       ((rew, done, torch.zeros(15, 8).t()), "contiguous"), ((rew.numpy(), done, st), "tensor is required"),
                       ((rew.to("meta"), done, st), "must live on"), ((rew, done.to("meta"), st), "must live on")):
        with pytest.raises(ValueError, match=what):
            m.record(*args)
    assert m.summary()["games"] == 0 and not m.cur.any()          # (a refused call changes nothing)
    m.record(rew, torch.tensor([True] + [False] * 7), st)         # a bool and a float done are cast
    m.record(rew.view(8, 1), torch.tensor([0.0, 1.0] + [0.0] * 6), st)
    s = m.summary()
    assert (s["games"], s["current_size"], s["mean_reward"], s["mean_rewards"], s["mean_length"]) == (2, 2, 1.5, [1.5, 0.0, 0.0], 1.5)
    assert sorted(s) == sorted(["current_size", "mean_reward", "mean_rewards", "mean_length", "games", "discarded", "window_mean_reward", "window_mean_length"])
    assert (s["window_mean_reward"], s["window_mean_length"], s["discarded"]) == (1.5, 1.5, 0)
    m.clear()
    assert m.summary()["games"] == 0 and m.summary()["current_size"] == 0


@pytest.mark.parametrize("cols", [1, 4])
def test_torch_backend_follows_the_restatement(cols):
    """backend="torch" is the same rule: sizes and counts exactly; means within the float64 test's bound per update (its sums are taken
    in float64, so its own error is the five roundings of the window update)."""
    n, max_size = 300, 100
    m, ref, syn = GM.GameMeter(n, "cpu", cols=cols, games_to_track=max_size, backend="torch"), MeterRef(n, cols, max_size), Synth(n, seed=5, p=0.1)
    updates, top = 0, 0.0
    for t in range(20):
        rew, stacked, done = syn.step()
        top = max(top, float(np.abs(rew).max()), float(np.abs(stacked[:, :cols]).max()))
        if t == 7:
            rew[3] = np.nan
        if t == 8:
            done[3] = 1
        m.record(torch.from_numpy(rew), torch.from_numpy(done), torch.from_numpy(stacked))
        updates += ref.record(rew, stacked, done) > 0
        assert np.array_equal(m.cur.numpy().view(np.uint32), ref.cur.view(np.uint32))
    s, r = m.summary(), unpack(ref.ms, cols)
    assert (s["current_size"], s["games"], s["discarded"]) == (r["current_size"], r["games"], r["discarded"]) and s["discarded"] == 1
    # (a return is at most 20 steps of the largest increment; a window mean is a convex combination, so errors add over the updates at most)
    tol = updates * (tree_depth() + groups(n) + 3) * U * 20 * max(top, 1.0)
    assert np.abs(np.asarray(s["mean_rewards"]) - r["mean"]).max() <= tol and abs(s["mean_length"] - r["mean_len"]) <= tol
    assert abs(s["window_mean_reward"] - r["sum_ret"] / r["games"]) <= tol


# ---------------------------------------------------------------------------------------------------- the walk learner's loop
def _ppo():
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(ROOT, "examples", "ppo_consumer.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class ShortEpisodes:
    """The VecTask surface train() touches, 64 envs on the CPU (DyrosDynamicWalk itself runs on the GPU only, so the episode length cannot
    come from its cfg here: tests/test_game_meter_gpu.py sets env.episodeLength).  Env i's episodes last 8 + i % 5 policy steps, so they end
    inside a rollout of 16; the reward grows with the epoch, so every epoch is a new best."""
    num_envs, num_obs, num_acts = 64, 12, 3

    def __init__(self, shrink=False):
        self.g = torch.Generator().manual_seed(100)
        self.extras = {}
        self.episodes_finished, self.epi_len_log = torch.zeros(64), torch.zeros(64)
        self.t, self.n, self.shrink = 0, torch.zeros(64, dtype=torch.int64), shrink
        self.fed = []

    def reset(self):
        return {"obs": torch.zeros(64, 12)}

    def step(self, a):
        self.t += 1
        self.n += 1
        done = (self.n >= 8 + torch.arange(64) % 5).long()
        self.n[done != 0] = 0
        o = torch.randn(64, 12, generator=self.g)
        epoch = (self.t - 1) // 16
        rew = torch.full((64,), 1.0 + (-0.25 if self.shrink else 0.25) * epoch) + 0.01 * torch.arange(64)
        self.fed.append((rew.clone(), done.clone()))
        return {"obs": o}, rew, done, {}


def test_cpu_training_run_with_the_meter(tmp_path):
    ppo = _ppo()
    from isaacgymdyros_amd import ppo_checkpoint as PK
    cfg = {"network": dict(ppo.TRAIN_CFG["network"], mlp_units=[16, 16]), "config": dict(ppo.TRAIN_CFG["config"], minibatch_size=256, mini_epochs=1)}
    kw = dict(device="cpu", num_envs=64, horizon=16, epochs=3, cfg=cfg)
    lines, env = [], ShortEpisodes()
    st = ppo.train(env=env, log=lines.append, game_meter=True, save_best_after=1, save_frequency=1, output_dir=str(tmp_path / "a"), **kw)
    gm = [s["game_meter"] for s in st]
    assert [g["games"] for g in gm] == sorted(g["games"] for g in gm) and gm[0]["games"] > 0 and gm[-1]["games"] > 100 and gm[-1]["current_size"] == 100
    # the meter saw what a plain replay of the steps gives (the torch backend on the CPU)
    replay = GM.GameMeter(64, "cpu", backend="torch")
    for rew, done in env.fed:
        replay.record(rew, done)
    assert replay.summary() == gm[-1]
    assert 8.0 <= gm[-1]["mean_length"] <= 12.0
    means = [g["mean_reward"] for g in gm]
    assert means == sorted(means) and means[0] < means[-1]          # every epoch a new best: <experiment>.pth each time, no last_ file but the final one
    nn_dir = tmp_path / "a" / "DyrosDynamicWalk" / "nn"
    final = "last_DyrosDynamicWalkep3rew%s.pth" % np.float32(means[-1])
    assert sorted(os.listdir(nn_dir)) == sorted(["DyrosDynamicWalk.pth", final])
    ck = torch.load(nn_dir / "DyrosDynamicWalk.pth", weights_only=True)
    assert ck["last_mean_rewards"] == max(means) == means[-1] and ck["epoch"] == 3 and list(ck)[:8] == PK.TOP_KEYS
    assert torch.load(nn_dir / final, weights_only=True)["last_mean_rewards"] == means[-1]
    assert sum(x.startswith("epoch") and "games: mean return" in x for x in lines) == 3

    # a run whose mean shrinks: the first epoch is the best, later save_frequency epochs are last_ files; <experiment>.pth keeps the best epoch
    lines_b, env_b = [], ShortEpisodes(shrink=True)
    st_b = ppo.train(env=env_b, log=lines_b.append, game_meter=True, save_best_after=1, save_frequency=1, output_dir=str(tmp_path / "b"), **kw)
    mb = [s["game_meter"]["mean_reward"] for s in st_b]
    assert mb[0] > mb[1] > mb[2]
    nn_b = tmp_path / "b" / "DyrosDynamicWalk" / "nn"
    assert sorted(os.listdir(nn_b)) == sorted(["DyrosDynamicWalk.pth", "last_DyrosDynamicWalk_ep_2_rew_%s.pth" % np.float32(mb[1]),
                                               "last_DyrosDynamicWalk_ep_3_rew_%s.pth" % np.float32(mb[2]), "last_DyrosDynamicWalkep3rew%s.pth" % np.float32(mb[2])])
    best = torch.load(nn_b / "DyrosDynamicWalk.pth", weights_only=True)
    assert best["epoch"] == 1 and best["last_mean_rewards"] == mb[0] == max(mb)
    # resuming from the best file starts with its value: an epoch below it is no new best, so <experiment>.pth is not written again
    lines_r = []
    env_r = ShortEpisodes(shrink=True)
    env_r.t = 16          # (it goes on where epoch 1 ended: smaller rewards)
    st_r = ppo.train(env=env_r, log=lines_r.append, game_meter=True, save_best_after=1, save_frequency=1, output_dir=str(tmp_path / "r"),
                     checkpoint=str(nn_b / "DyrosDynamicWalk.pth"), **dict(kw, epochs=1))
    assert st_r[0]["epoch"] == 2 and st_r[0]["game_meter"]["mean_reward"] < mb[0]
    nn_r = tmp_path / "r" / "DyrosDynamicWalk" / "nn"
    assert "DyrosDynamicWalk.pth" not in os.listdir(nn_r) and len(os.listdir(nn_r)) == 2
    for f in os.listdir(nn_r):
        assert f.startswith("last_") and torch.load(nn_r / f, weights_only=True)["last_mean_rewards"] == mb[0]

    # without the switch: the stats dicts, the log lines and the files are what they are without this feature
    lines_off = []
    off = ppo.train(env=ShortEpisodes(), log=lines_off.append, save_frequency=1, output_dir=str(tmp_path / "off"), **kw)
    assert all("game_meter" not in s for s in off) and len(lines_off) == 3 and not any("games:" in x for x in lines_off)
    assert sorted(os.listdir(tmp_path / "off" / "DyrosDynamicWalk" / "nn")) == ["DyrosDynamicWalk.pth", "DyrosDynamicWalk_1.pth", "DyrosDynamicWalk_2.pth", "DyrosDynamicWalk_3.pth"]
    assert torch.load(tmp_path / "off" / "DyrosDynamicWalk" / "nn" / "DyrosDynamicWalk.pth", weights_only=True)["last_mean_rewards"] == -100500
    keys = lambda s: sorted(k for k in s if k != "game_meter")          # noqa: E731
    assert [keys(s) for s in off] == [keys(s) for s in st]
    for a, b in zip(off, st):          # (same seeds, same env: the meter changes nothing the loop computes)
        assert a["mean_reward"] == b["mean_reward"] and a["a_loss"] == b["a_loss"] and a["frame"] == b["frame"]
    assert [x.split("mean reward")[1] for x in lines if "games:" not in x] == [x.split("mean reward")[1] for x in lines_off]
