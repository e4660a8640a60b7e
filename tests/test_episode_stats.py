"""Episode statistics without a GPU (include/dyros_stats.h, isaacgymdyros_amd/csrc/dw_stats.h): the per-env update
and the reduction -- compiled by g++ from the same header the HIP kernels include (tests/stats_host.cpp) -- against the numpy restatement of tests/episode_stats_ref.py on synthetic buffers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from isaacgymdyros_amd import abi
from isaacgymdyros_amd import episode_stats as S
from episode_stats_ref import StatsRef, compare_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, E = S.K, abi.K
NB, ESW = E["DW_NUM_BODIES"], E["DW_ES_WORDS"]
ML, DTP = 40.0, 0.004          # a short episode so that time limits fall inside a test


def test_layout_constants_fit():
    assert K["DWS_CT_BODY"] + NB <= K["DWS_CT_BIN_EP"]
    assert K["DWS_CT_LEN_HIST"] + K["DWS_LEN_BINS"] <= K["DWS_CT_BODY"]
    assert K["DWS_CT_PUSH_FALLS"] < K["DWS_CT_WINDOW"] <= K["DWS_CT_CALLS"] < K["DWS_CT_GATE_AT"] < K["DWS_CT_WORDS"]
    assert K["DWS_AC_RATIO"] + K["DWS_CMD_BINS"] == K["DWS_AC_WORDS"]
    assert K["DWS_SUM_WORDS"] == K["DWS_CT_WORDS"] + K["DWS_AC_WORDS"]


def test_validate_cfg_checks_the_switch():
    from isaacgymdyros_amd.config import default_cfg, validate_cfg
    cfg = default_cfg(8, "cpu")
    validate_cfg(cfg)
    cfg["sim"]["mi355"]["episode_stats"] = True
    validate_cfg(cfg)
    cfg["sim"]["mi355"]["episode_stats"] = 1
    with pytest.raises(ValueError, match="episode_stats"):
        validate_cfg(cfg)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/stats_host.cpp")
    so = str(tmp_path_factory.mktemp("dwsh") / "libdwsh.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, os.path.join(ROOT, "tests", "stats_host.cpp")])
    lib = C.CDLL(so)
    P, I, F = C.c_void_p, C.c_int32, C.c_float
    lib.dwsh_record.argtypes = [I, P, P, P, P, P, P, P, P, P, F, F]
    lib.dwsh_restart.argtypes = [I, P, I, P, P, P, P]
    lib.dwsh_summarize.argtypes = [I, P, P, P]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Pair:
    """The g++ build and the numpy restatement, driven with the same buffers."""

    def __init__(self, host, n, max_len=ML):
        self.h, self.n, self.ml = host, n, max_len
        self.st = np.zeros((K["DWS_ST_WORDS"], n), np.uint32)
        self.ac = np.zeros((K["DWS_AC_WORDS"], n), np.float32)
        self.ct = np.zeros(K["DWS_CT_WORDS"], np.uint64)
        self.ref = StatsRef(n, max_len, DTP)
        self.root = np.zeros((n, 13), np.float32)
        self.root[:, 2] = 0.9
        self.root[:, 6] = 1.0
        self.cf = np.zeros((n, NB, 3), np.float32)
        self.es = np.zeros((n, ESW), np.float32)
        self.esi = self.es.view(np.int32)
        self.mass = np.full(n, 100.0, np.float32)
        self.progress = np.zeros(n, np.int64)
        self.restart()

    def restart(self, ids=None):
        a = None if ids is None else np.ascontiguousarray(ids, np.int32)
        self.h.dwsh_restart(self.n, None if a is None else _p(a), 0 if a is None else a.size, _p(self.root), _p(self.es), _p(self.progress), _p(self.st))
        self.ref.restart(self.root, self.es, self.progress, ids)

    def step(self, reset):
        reset = np.ascontiguousarray(reset, np.int64)
        cause = np.zeros(self.n, np.uint8)
        self.h.dwsh_record(self.n, _p(self.root), _p(self.cf), _p(self.es), _p(reset), _p(self.mass), _p(self.st), _p(self.ac), _p(self.ct),
                           _p(cause), self.ml, DTP)
        want = self.ref.record(self.root, self.cf, self.es, reset, self.mass)
        assert (cause == want).all(), (cause, want)
        assert (self.st == self.ref.st).all(), np.nonzero(self.st != self.ref.st)
        assert (self.ac == self.ref.ac).all()
        assert (self.ct.astype(np.int64) == self.ref.ct).all(), np.nonzero(self.ct.astype(np.int64) != self.ref.ct)
        return cause

    def summary(self):
        out = np.zeros(K["DWS_SUM_WORDS"], np.float64)
        self.h.dwsh_summarize(self.n, _p(self.ac), _p(self.ct), _p(out))
        compare_raw(out, self.ref.raw(), rtol=1e-12)
        return S.fold(out.tolist(), self.n, self.ml, ["b%d" % g for g in range(NB)])

    def walk(self, k):
        """k steps without a reset: the robots creep forward at the commanded speed."""
        for _ in range(k):
            self.root[:, 0] += self.es[:, E["DW_ES_TARGET_VEL"]] * DTP
            self.root[:, 7] = self.es[:, E["DW_ES_TARGET_VEL"]] * 0.9
            self.step(np.zeros(self.n))


def test_each_cause_on_its_own(host):
    p = Pair(host, 5)
    p.walk(3)
    p.esi[0, E["DW_ES_NAN_RESETS"]] += 1                      # non_finite (the step zeroes the env's contact row)
    p.cf[1, 5] = (0.0, 0.0, 30.0)                            # non_foot_contact
    p.ref.si[K["DWS_ST_N"], 2] = p.st[K["DWS_ST_N"], 2] = int(ML) - 2          # time_limit: n = ML - 1 at this step
    cause = p.step([1, 1, 1, 1, 0])                          # env 3: nothing else -> orientation; env 4 did not reset
    assert list(cause) == [4, 2, 1, 3, 0]
    s = p.summary()
    assert s["episodes"] == 4 and s["causes"] == {"time_limit": 1, "non_foot_contact": 1, "orientation": 1, "non_finite": 1}
    assert s["contact_bodies"] == {"b5": 1}


def test_precedence_pairs(host):
    p = Pair(host, 3)
    p.walk(2)
    p.esi[0, E["DW_ES_NAN_RESETS"]] = 7                      # NaN + contact -> non_finite
    p.cf[0, 3] = (5.0, 0.0, 0.0)
    p.cf[1, 30] = (0.0, -4.0, 0.0)                           # contact + time limit -> non_foot_contact
    for e in (1, 2):                                         # time limit + orientation (the rest of the OR) -> time_limit
        p.ref.si[K["DWS_ST_N"], e] = p.st[K["DWS_ST_N"], e] = int(ML)
    assert list(p.step([1, 1, 1])) == [4, 2, 1]
    assert p.summary()["contact_bodies"] == {"b30": 1}       # the body of the NaN env is not counted: its episode is non_finite


def test_time_limit_uses_the_stats_own_step_count(host):
    p = Pair(host, 2)
    p.progress[:] = [int(ML) - 3, int(ML) - 4]               # an explicit restart picks the count up from progress_buf
    p.restart()
    p.walk(1)
    assert list(p.step([1, 1])) == [1, 3]                    # n = ML - 1 and ML - 2


def test_body_histogram(host):
    p = Pair(host, 4)
    p.walk(1)
    p.cf[0, 3] = (0.0, 0.0, 2.0)
    p.cf[0, 20] = (1.5, 0.0, 0.0)
    p.cf[0, 8] = (0.0, 0.0, 900.0)                           # a sole: never a contact cause
    p.cf[1, 20] = (0.0, 0.0, 3.0)
    p.cf[1, 37] = (0.0, 0.0, 0.5)                            # under 1 N
    p.cf[2, 16] = (0.0, 0.0, 2000.0)                         # the other sole: env 2 ends by orientation
    p.cf[3, 0] = (0.0, 0.0, 9.0)                             # env 3 does not reset: its contact is no cause
    assert list(p.step([1, 1, 1, 0])) == [2, 2, 3, 0]
    s = p.summary()
    assert s["contact_bodies"] == {"b3": 1, "b20": 2}
    assert s["sole_over_1400"] == [0.0, 1 / 3]


@pytest.mark.parametrize("gap,falls", [(249, 1), (251, 0)])
def test_push_window(host, gap, falls):
    """An episode that ends (not by time limit) `gap` steps after the last step with pert_on set: a push fall up to 250."""
    p = Pair(host, 2, max_len=10000.0)
    p.walk(2)
    p.esi[:, E["DW_ES_PERT_ON"]] = 1
    p.walk(3)
    p.esi[:, E["DW_ES_PERT_ON"]] = 0
    p.walk(gap - 1)
    p.esi[0, E["DW_ES_PERT_ON"]] = 0
    assert list(p.step([1, 0])) == [3, 0]
    s = p.summary()
    assert s["pushes"] == 2 and s["push_falls"] == falls


def test_terminal_step_rule(host):
    """Root states of the terminal step are the new episode's and are skipped; contact forces and torques of that step count."""
    p = Pair(host, 2)
    p.es[:, E["DW_ES_TARGET_VEL"]] = 0.5
    p.restart()
    p.walk(40)                                               # (0.5 m/s for 40 steps of 4 ms: 0.08 m, over DWS_RATIO_MIN_M)
    x_end = p.root[:, 0].copy()
    p.root[:, :2] = (50.0, -50.0)                            # the reset pose: far away
    p.root[:, 7] = 9.0
    p.es[:, E["DW_ES_TARGET_VEL"]] = 0.1                     # the new episode's command
    p.cf[:, 8, 2] = 1500.0                                   # the terminal step's sole load
    p.es[:, E["DW_ES_ACTION_TORQUE"]:E["DW_ES_ACTION_TORQUE"] + 12] = 3.0
    p.step([1, 1])
    s = p.summary()
    b = s["command_bins"][2]                                 # the episode's command, 0.5, not the new one
    assert b["episodes"] == 2 and s["command_bins"][0]["episodes"] == 0
    assert b["vel_error"] == pytest.approx(0.05, rel=1e-5)
    assert b["lateral_drift"] == 0.0
    assert b["distance_ratio"] == pytest.approx(1.0, rel=1e-4) and x_end[0] == pytest.approx(0.08, rel=1e-4)
    assert s["sole_peak_mean"][0] == 1500.0 and s["sole_over_1400"][0] == 1.0
    assert s["torque_diff_max_mean"] == 3.0                  # the terminal step's torque against the previous record's (0): it counts
    assert s["torque_mean"] == pytest.approx(3.0 / 41, rel=1e-6)
    # the new episode starts from the reset pose
    assert p.ref.sf[K["DWS_ST_X0"], 0] == 50.0 and p.ref.sf[K["DWS_ST_TV0"], 0] == np.float32(0.1)


def test_torque_difference_of_consecutive_records(host):
    """The step kernel has copied this step's action_torque into action_torque_pre before a record runs (its late update), as here: the
    difference is taken against the previous record's action_torque, from the second record of an episode on, terminal step included."""
    p = Pair(host, 3)
    seq = [[1.0, 5.0, 2.0, -4.0, -4.0], [0.0, 0.0, 0.0, 0.0, 0.0], [7.0, 7.5, 7.0, 6.0, 9.0]]          # per env: the torque of joint 3 per record
    for t in range(5):
        tq = np.zeros((3, 12), np.float32)
        tq[:, 3] = [seq[e][t] for e in range(3)]
        tq[2, 0] = -2.0 * t                                  # env 2: another joint jumps by 2 per record
        p.es[:, E["DW_ES_ACTION_TORQUE"]:E["DW_ES_ACTION_TORQUE"] + 12] = tq
        p.es[:, E["DW_ES_ACTION_TORQUE_PRE"]:E["DW_ES_ACTION_TORQUE_PRE"] + 12] = tq          # (what a real step leaves)
        p.step([0, 0, 0] if t < 4 else [1, 1, 1])
    s = p.summary()
    # env 0: |5-1|, |2-5|, |-4-2|, |-4+4| -> 6; env 1: 0; env 2: max(0.5, 0.5, 1, 3; joint 0: 2) -> 3
    assert s["torque_diff_max_mean"] == pytest.approx((6.0 + 0.0 + 3.0) / 3)
    # a new episode starts without a previous torque: its first record adds no difference
    p.step([0, 0, 0])
    assert p.ref.sf[K["DWS_ST_DTM"]].tolist() == [0.0, 0.0, 0.0]
    tq = np.full((3, 12), 50.0, np.float32)
    p.es[:, E["DW_ES_ACTION_TORQUE"]:E["DW_ES_ACTION_TORQUE"] + 12] = tq
    p.step([0, 0, 0])
    assert p.ref.sf[K["DWS_ST_DTM"]].tolist() == [54.0, 50.0, 58.0]          # against the first record's -4, 0, 9 and -8


def test_restart_discards_the_running_episode(host):
    p = Pair(host, 4)
    p.walk(5)
    p.cf[:, 2] = (0.0, 0.0, 40.0)
    p.walk(1)                                                # contact while running: no cause until a reset
    p.cf[:] = 0.0
    p.progress[:] = 0
    p.restart([1, 3])                                        # env 1 and 3 start over
    p.walk(2)
    p.step([1, 1, 1, 1])
    s = p.summary()
    assert s["episodes"] == 4
    assert s["length_hist"][3] == 2 and s["length_hist"][1] == 2 and s["max_length"] == 9          # (16 bins over [0, 40])
    assert s["mean_length"] == (9 + 3 + 9 + 3) / 4


def test_random_sequence_and_windows(host):
    """Random buffers for 300 records of 37 envs (a last workgroup of fewer envs on the GPU), two windows, restarts in between."""
    rng = np.random.default_rng(5)
    n = 37
    p = Pair(host, n, max_len=60.0)
    p.es[:, E["DW_ES_TARGET_VEL"]] = rng.uniform(0, 0.8, n)
    p.restart()
    for t in range(300):
        p.root[:] = rng.normal(0, 1, p.root.shape).astype(np.float32)
        p.cf[:] = rng.normal(0, 1, p.cf.shape).astype(np.float32) * (rng.random((n, NB, 1)) < 0.02) * 30
        p.cf[:, 8, 2] = rng.uniform(0, 1600, n)
        p.cf[:, 16, 2] = rng.uniform(0, 1600, n)
        p.es[:, E["DW_ES_TARGET_FORCE"]:E["DW_ES_TARGET_FORCE"] + 2] = rng.normal(0, 5, (n, 2))
        p.es[:, E["DW_ES_ACTION_TORQUE"]:E["DW_ES_ACTION_TORQUE"] + 24] = rng.normal(0, 20, (n, 24))
        p.es[:, E["DW_ES_LAST_RETURN"]] = rng.normal(0, 10, n)
        p.esi[:, E["DW_ES_PERT_ON"]] = rng.random(n) < 0.1
        p.esi[:, E["DW_ES_NAN_RESETS"]] += rng.random(n) < 0.01
        p.esi[0, E["DW_ES_PERT_START"]] = int(t >= 120)
        reset = (rng.random(n) < 0.05) | (p.ref.si[K["DWS_ST_N"]] + 1 >= 59)
        p.es[reset, E["DW_ES_TARGET_VEL"]] = rng.uniform(0, 0.8, int(reset.sum()))
        p.step(reset)
        if t == 150:
            p.summary()
            p.ac[:] = 0
            p.ct[:K["DWS_CT_WINDOW"]] = 0
            p.ref.reset_totals()
        if t in (90, 200):
            ids = rng.choice(n, 5, replace=False)
            p.progress[ids] = rng.integers(0, 50, 5)
            p.restart(ids)
    s = p.summary()
    assert s["records"] == 149 and s["record_calls"] == 300
    assert s["perturb_start_latched"] and s["perturb_start_at_record"] == 120
    assert sum(s["causes"].values()) == s["episodes"] > 0
    assert all(v > 0 for v in s["causes"].values())
