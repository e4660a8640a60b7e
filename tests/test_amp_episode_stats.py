"""TocabiAMPLower's episode statistics without a GPU (include/dyros_amp_stats.h, isaacgymdyros_amd/csrc/dw_amp_stats.h):
the per-env update and the reduction -- compiled by g++ from the same header the HIP kernels include (tests/amp_stats_host.cpp) -- against the
numpy restatement of tests/amp_episode_stats_ref.py on synthetic buffers; the layout, the cfg key and the kernels' scratch."""
import copy
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from isaacgymdyros_amd import amp_episode_stats as S
from amp_episode_stats_ref import AmpStatsRef, cause_mask, compare_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = S.K
NB = K["DWE_BODIES"]
ML, TH, LO, HI = 40.0, 0.6, -0.5, 1.0          # a short episode so that time limits fall inside a test
T, CO, LW, FL, TI = (K["DWE_C_" + n] for n in ("TIME", "CONTACT", "LOW", "FLY", "TILT"))
FLOAT_ST = [K["DWE_ST_RET"], K["DWE_ST_PKL"], K["DWE_ST_PKR"]]


def test_layout_constants_do_not_overlap():
    st = sorted(v for k, v in K.items() if k.startswith("DWE_ST_") and k != "DWE_ST_WORDS")
    assert st == list(range(K["DWE_ST_WORDS"]))
    ac = [("RET", 1), ("REW", K["DWE_REW_TERMS"]), ("VERR", K["DWE_CMD_BINS"]), ("VCNT", K["DWE_CMD_BINS"]), ("YAW", 1), ("PK", 2)]
    ct = [("RECORDS", 1), ("EPISODES", 1), ("DISCARDED", 1), ("UNRESET", 1), ("NONFINITE", 1), ("SAMPLES", 1), ("MASK", K["DWE_MASKS"]),
          ("LEN_SUM", 1), ("LEN_MAX", 1), ("LEN_HIST", K["DWE_LEN_BINS"]), ("BODY", NB), ("SOLE_OVER", 2)]
    for pre, fields, end in (("DWE_AC_", ac, K["DWE_AC_WORDS"]), ("DWE_CT_", ct, K["DWE_CT_WINDOW"])):
        at = 0
        for name, size in fields:
            assert K[pre + name] == at, (pre + name, at)
            at += size
        assert at == end
    assert K["DWE_CT_WINDOW"] == K["DWE_CT_CALLS"] < K["DWE_CT_WORDS"]
    assert K["DWE_MASKS"] == 2 * max(T, CO, LW, FL, TI) and sorted((T, CO, LW, FL, TI)) == [1, 2, 4, 8, 16]
    assert K["DWE_SUM_WORDS"] == K["DWE_CT_WORDS"] + K["DWE_AC_WORDS"]
    assert S.EXPORTS == ["abi_version", "last_error", "record", "summarize"]


def test_bindings_come_from_the_header():
    """The sixth C ABI, held to what tests/test_cbind.py holds the other five to: the names bound are the header's, the built library exports
    each and reports the header's version, and every prototype has the header's arguments in kind and place."""
    import test_cbind as TC
    from isaacgymdyros_amd import build
    TC.test_ctypes_prototypes_match_the_header("dyros_amp_stats.h", "dwe_", "amp_episode_stats", C.CDLL(build.build()))
    src = open(os.path.join(ROOT, "isaacgymdyros_amd", "amp_episode_stats.py")).read()
    assert "argtypes" not in src and "restype" not in src          # (no hand-written prototypes)


# ---------------------------------------------------------------------------------------------- the cfg key
class _Stop(Exception):
    pass


def _construct(monkeypatch, mi):
    """TocabiAMPLower's constructor up to the physics host, which is replaced by a stub that keeps the cfg it was handed."""
    from isaacgymdyros_amd import tocabi_amp_lower as tal
    seen = {}

    def host(cfg, *a, **k):
        seen["cfg"] = copy.deepcopy(cfg)
        raise _Stop()
    monkeypatch.setattr(tal, "DyrosDynamicWalk", host)
    cfg = tal.default_amp_cfg(8, "cuda:0")
    cfg["sim"]["mi355"] = dict(mi)
    with pytest.raises(_Stop):
        tal.TocabiAMPLower(cfg, "cuda:0", 0, True)
    return seen["cfg"]


def test_cfg_key_must_be_a_bool(monkeypatch):
    from isaacgymdyros_amd import tocabi_amp_lower as tal
    for bad in (1, 0, "yes", None):
        cfg = tal.default_amp_cfg(8, "cuda:0")
        cfg["sim"]["mi355"] = {"amp_episode_stats": bad}
        with pytest.raises(ValueError, match="amp_episode_stats"):
            tal.TocabiAMPLower(cfg, "cuda:0", 0, True)


def test_cfg_key_does_not_reach_the_physics_host(monkeypatch):
    inner = _construct(monkeypatch, {"amp_episode_stats": True, "amp_fused": True})
    assert "amp_episode_stats" not in inner["sim"]["mi355"]
    assert not inner["sim"]["mi355"].get("episode_stats", False)          # (the walk's statistics stay off in the host)
    assert inner["sim"]["mi355"]["amp_fused"] is True                      # (the other keys travel as before)
    # `episode_stats` in a TocabiAMPLower cfg is the host's key and is handed on unchanged, as before this feature
    assert _construct(monkeypatch, {"episode_stats": True})["sim"]["mi355"]["episode_stats"] is True


# ---------------------------------------------------------------------------------------------- the g++ build against numpy
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/amp_stats_host.cpp")
    so = str(tmp_path_factory.mktemp("dweh") / "libdweh.so")
    # (dw_amp_stats.h includes the product's device-only headers: the host shims of tests/emul stand in, as in tests/emul/Makefile)
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-strict-aliasing",
                           "-I" + os.path.join(ROOT, "tests", "emul"), '-DDWQ_HOST_SHIM_HEADER="dw_quad_wave_host.h"',
                           '-DDW_HOST_SHIM_HEADER="dw_wave_host.h"', "-o", so, os.path.join(ROOT, "tests", "amp_stats_host.cpp")])
    lib = C.CDLL(so)
    P, I, F = C.c_void_p, C.c_int32, C.c_float
    lib.dweh_record.argtypes = [I] + [P] * 13 + [F, F, I, F, F]
    lib.dweh_summarize.argtypes = [I, P, P, P]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def close(got, want, rtol=1e-6):
    """The issue's bound for float words: rtol relative to max(|want|, 1e-3)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool((np.abs(got - want) <= rtol * np.maximum(np.abs(want), 1e-3)).all())


class Pair:
    """The g++ build and the numpy restatement, driven with the same buffers.  The envs stand upright on their soles unless a test says otherwise."""

    def __init__(self, host, n, max_len=ML, eet=True):
        self.h, self.n, self.ml, self.eet = host, n, max_len, eet
        self.st = np.zeros((K["DWE_ST_WORDS"], n), np.uint32)
        self.st.view(np.int32)[K["DWE_ST_N"]] = -1
        self.ac = np.zeros((K["DWE_AC_WORDS"], n), np.float32)
        self.ct = np.zeros(K["DWE_CT_WORDS"], np.uint64)
        self.ref = AmpStatsRef(n, max_len, TH, eet, LO, HI)
        self.root = np.zeros((n, 13), np.float32)
        self.root[:, 2] = 0.93
        self.root[:, 6] = 1.0
        self.cf = np.zeros((n, NB, 3), np.float32)
        self.cf[:, (8, 16), 2] = 500.0
        self.rbp = np.zeros((n, NB, 3), np.float32)
        self.rbp[:, (8, 16), 2] = 0.08
        self.cmd = np.zeros((n, 3), np.float32)
        self.rew = np.full(n, 0.5, np.float32)
        self.rv = np.tile(np.arange(1, 10, dtype=np.float32) * np.float32(0.01), (n, 1))
        self.mass = np.full(n, 100.0, np.float32)
        self.progress = np.zeros(n, np.int64)

    def restart(self, ids=None):
        self.st.view(np.int32)[K["DWE_ST_N"], slice(None) if ids is None else np.asarray(ids)] = -1
        self.ref.restart(ids)

    def step(self, reset=None, advance=True):
        """One record; progress_buf is incremented first, as the step does.  reset None: the step's own flag (any cause bit)."""
        if advance:
            self.progress += 1
        cause = np.zeros(self.n, np.uint8)
        if reset is None:
            reset = cause_mask(self.root, self.cf, self.rbp, self.progress, self.ml, TH, self.eet) != 0
        want = self.ref.record(self.root, self.cf, self.rbp, self.cmd, self.rew, self.rv, reset, self.progress, self.mass)
        reset = np.ascontiguousarray(reset, np.int64)
        self.h.dweh_record(self.n, _p(self.root), _p(self.cf), _p(self.rbp), _p(self.cmd), _p(self.rew), _p(self.rv), _p(reset), _p(self.progress),
                           _p(self.mass), _p(self.st), _p(self.ac), _p(self.ct), _p(cause), self.ml, TH, int(self.eet), LO, HI)
        assert (cause == want).all(), (cause, want)
        isw = [k for k in range(K["DWE_ST_WORDS"]) if k not in FLOAT_ST]
        assert (self.st[isw] == self.ref.st[isw]).all(), np.nonzero(self.st[isw] != self.ref.st[isw])
        assert close(self.st.view(np.float32)[FLOAT_ST], self.ref.sf[FLOAT_ST])
        assert close(self.ac, self.ref.ac)
        assert (self.ct.astype(np.int64) == self.ref.ct).all(), np.nonzero(self.ct.astype(np.int64) != self.ref.ct)
        return cause

    def reset_done(self, ids):
        self.progress[np.asarray(ids)] = 0

    def summary(self):
        out = np.zeros(K["DWE_SUM_WORDS"], np.float64)
        self.h.dweh_summarize(self.n, _p(self.ac), _p(self.ct), _p(out))
        compare_raw(out, self.ref.raw(), rtol=1e-6)
        return S.fold(out.tolist(), self.ml, ["b%d" % g for g in range(NB)], (LO, HI))


def tilt(p, e, rad=1.0):
    p.root[e, 3:7] = (np.sin(rad / 2), 0.0, 0.0, np.cos(rad / 2))


def test_every_cause_bit_alone(host):
    p = Pair(host, 6)
    for _ in range(3):
        assert not p.step().any()
    p.cf[0, 5] = (0.0, 0.0, 30.0)                            # CONTACT
    p.root[1, 2] = 0.55                                      # LOW
    p.rbp[2, 16, 2] = 0.51                                   # FLY (the right foot)
    tilt(p, 3)                                               # TILT: 1 rad > pi / 4
    p.progress[4] = int(ML) - 2                              # TIME at this step: p = ML - 1 (seen as an outside jump: a new episode)
    cause = p.step()                                         # env 5: nothing
    assert list(cause) == [CO, LW, FL, TI, T, 0]
    s = p.summary()
    assert s["episodes"] == 5 and s["discarded"] == 1
    assert s["causes"] == {"time_limit": 1, "non_foot_contact": 1, "root_low": 1, "foot_high": 1, "tilt": 1}
    assert s["cause_masks"] == {"time_limit": 1, "non_foot_contact": 1, "root_low": 1, "foot_high": 1, "tilt": 1}
    assert s["contact_bodies"] == {"b5": 1}
    assert s["max_length"] == int(ML) - 1 and s["mean_length"] == (4 * 4 + int(ML) - 1) / 5


def test_cause_bits_combined(host):
    p = Pair(host, 4)
    for _ in range(2):
        p.step()
    p.cf[0, 3] = (5.0, 0.0, 0.0)
    p.cf[0, 30] = (0.0, 1.5, 0.0)
    p.root[0, 2] = 0.2
    tilt(p, 0, 2.0)                                          # CONTACT + LOW + TILT
    p.rbp[1, 8, 2] = 0.7
    p.rbp[1, 16, 2] = 0.9
    p.root[1, 2] = 0.59                                      # FLY + LOW
    for e in (2, 3):
        p.cf[e, 0] = (0.0, 0.0, 2.0)
    p.rbp[3, 8, 2] = 3.0
    p.root[3, 2] = -1.0
    tilt(p, 3, 3.0)                                          # all four
    cause = p.step()
    assert list(cause) == [CO | LW | TI, FL | LW, CO, CO | LW | FL | TI]
    s = p.summary()
    assert s["cause_masks"] == {"non_foot_contact+root_low+tilt": 1, "root_low+foot_high": 1, "non_foot_contact": 1,
                                "non_foot_contact+root_low+foot_high+tilt": 1}
    assert s["causes"] == {"time_limit": 0, "non_foot_contact": 3, "root_low": 3, "foot_high": 2, "tilt": 2}
    assert s["contact_bodies"] == {"b3": 1, "b30": 1, "b0": 2}


def test_contact_is_by_component_and_never_a_sole(host):
    p = Pair(host, 5)
    for _ in range(2):
        p.step()
    p.cf[0, 4] = (0.9, 0.9, 0.9)                             # norm 1.56, no component over 1: no contact
    p.cf[1, 4] = (-50.0, -50.0, -50.0)                       # negative components: no contact
    p.cf[2, 4] = (0.0, 1.0000001, 0.0)                       # just over
    p.cf[3, 8] = (0.0, 0.0, 2000.0)                          # a sole
    p.cf[4, 16] = (30.0, 0.0, 2000.0)                        # the other sole
    assert list(p.step()) == [0, 0, CO, 0, 0]
    s = p.summary()
    assert s["contact_bodies"] == {"b4": 1}
    # 1.4 * 9.81 * 100 = 1373.4: envs 3 and 4 were over it for one sampled step each, of 15 sampled steps
    assert s["sole_over_threshold"] == [1 / 15, 1 / 15]


def test_the_first_step_of_an_episode_cannot_fall(host):
    """fallen && progress_buf > 1: at p = 1 no early-termination bit is set, at p = 2 all of them are."""
    p = Pair(host, 2)
    p.cf[:, 2] = (0.0, 0.0, 40.0)
    p.root[:, 2] = 0.1
    p.rbp[:, 8, 2] = 0.6
    tilt(p, 0)
    tilt(p, 1)
    assert list(p.step()) == [0, 0]
    assert list(p.step()) == [CO | LW | FL | TI] * 2
    assert p.summary()["mean_length"] == 2.0


def test_early_termination_off(host):
    p = Pair(host, 2, eet=False)
    p.step()
    p.cf[:, 2] = (0.0, 0.0, 40.0)
    p.root[:, 2] = 0.1
    tilt(p, 0)
    for _ in range(5):
        assert list(p.step()) == [0, 0]
    p.progress[:] = int(ML) - 2
    p.restart()
    assert list(p.step()) == [T, T]
    s = p.summary()
    assert s["episodes"] == 2 and s["causes"]["time_limit"] == 2 and sum(s["causes"].values()) == 2 and not s["contact_bodies"]


def test_time_limit_together_with_a_fall(host):
    p = Pair(host, 3, max_len=6.0)
    for _ in range(4):
        assert not p.step().any()
    p.cf[0, 7] = (0.0, 0.0, 9.0)
    tilt(p, 1)
    cause = p.step()                                         # p = 5 >= 6 - 1
    assert list(cause) == [T | CO, T | TI, T]
    s = p.summary()
    assert s["cause_masks"] == {"time_limit+non_foot_contact": 1, "time_limit+tilt": 1, "time_limit": 1}
    assert s["contact_bodies"] == {"b7": 1}
    assert s["length_hist"][13] == 3 and sum(s["length_hist"]) == 3          # (5 * 16 / 6 = 13.3)
    assert s["mean_return"] == pytest.approx(2.5, rel=1e-6)


def test_adoption_in_mid_episode(host):
    """A record that starts while episodes run (construction, restart): the first record adopts the episode; its length is progress_buf, its
    return and peaks what the statistics saw of it."""
    p = Pair(host, 2)
    p.progress[:] = [10, 20]
    p.step()
    p.step()
    p.cf[0, 8, 2] = 981.0                                    # 1.0 x weight
    p.step()
    p.cf[0, 8, 2] = 500.0
    p.root[:, 2] = 0.3
    assert list(p.step()) == [LW, LW]
    s = p.summary()
    assert s["episodes"] == 2 and s["discarded"] == 0
    assert s["mean_length"] == (14 + 24) / 2 and s["mean_return"] == pytest.approx(4 * 0.5, rel=1e-6)
    assert s["sole_peak_mean"][0] == pytest.approx((1.0 + 500.0 / 981.0) / 2, rel=1e-6)


def test_an_outside_reset_discards_the_running_episode(host):
    p = Pair(host, 4)
    for _ in range(5):
        p.step()
    p.reset_done([1, 3])                                     # reset_idx in mid-episode: progress_buf goes back to 0
    for _ in range(2):
        p.step()
    p.root[:, 2] = 0.2
    assert list(p.step()) == [LW] * 4
    s = p.summary()
    assert s["episodes"] == 4 and s["discarded"] == 2
    assert s["mean_length"] == (8 + 3 + 8 + 3) / 4
    assert s["mean_return"] == pytest.approx((8 + 3 + 8 + 3) * 0.5 / 4, rel=1e-6)          # the discarded steps' rewards are gone
    p.restart([0])                                           # restart() forgets without counting
    p.reset_done([0, 1, 2, 3])
    p.root[:, 2] = 0.93
    p.step()
    assert p.summary()["discarded"] == 2


def test_an_env_the_caller_does_not_reset(host):
    p = Pair(host, 3)
    for _ in range(3):
        p.step()
    p.root[0, 2] = 0.2
    assert list(p.step()) == [LW, 0, 0]
    ac0 = p.ac.copy()
    for _ in range(4):                                       # env 0 stays down and is never reset: its mask stays, nothing is added
        assert list(p.step()) == [LW, 0, 0]
    assert (p.ac[:, 0] == ac0[:, 0]).all()
    s = p.summary()
    assert s["episodes"] == 1 and s["unreset_steps"] == 4 and s["sampled_steps"] == 3 * 8 - 4
    p.reset_done([0])                                        # reset late: a new episode, no discard
    p.root[0, 2] = 0.93
    p.step()
    s = p.summary()
    assert s["discarded"] == 0 and s["unreset_steps"] == 4 and p.ref.si[K["DWE_ST_N"], 0] == 1


def test_a_non_finite_row_adds_to_no_float_sum(host):
    p = Pair(host, 3)
    for _ in range(2):
        p.step()
    p.root[1, 8] = np.nan
    p.rew[1] = np.nan
    p.rv[1] = np.inf
    p.step(reset=[0, 0, 0])
    p.root[1, 8] = 0.0
    p.root[1, 0] = -np.inf
    p.step(reset=[0, 1, 0])                                  # it ends on a non-finite step: counted, with what it had
    s = p.summary()
    assert np.isfinite(p.ac).all() and np.isfinite(p.st.view(np.float32)[FLOAT_ST]).all()
    assert s["nonfinite_steps"] == 2 and s["sampled_steps"] == 3 * 4 - 2
    assert s["episodes"] == 1 and s["mean_length"] == 4.0 and s["mean_return"] == pytest.approx(1.0, rel=1e-6)
    assert all(np.isfinite(v) for v in s["reward_terms"].values())


def test_command_bins_are_per_step(host):
    p = Pair(host, 2)
    p.root[:, 7] = 0.25                                      # upright: local v_x = v_x
    for c in (-0.5, -0.2, 0.1, 0.2, 0.7, 1.0, 1.4, -2.0):    # bins of width 0.375 from -0.5
        p.cmd[:, 0] = c
        p.cmd[:, 2] = 0.1
        p.step()
    s = p.summary()
    assert [b["steps"] for b in s["command_bins"]] == [6, 4, 0, 6]
    assert [b["lo"] for b in s["command_bins"]] == [-0.5, -0.125, 0.25, 0.625]
    assert s["command_bins"][0]["x_vel_error"] == pytest.approx((0.75 + 0.45 + 2.25) / 3, rel=1e-6)
    assert s["command_bins"][1]["x_vel_error"] == pytest.approx((0.15 + 0.05) / 2, rel=1e-5)
    assert np.isnan(s["command_bins"][2]["x_vel_error"])
    assert s["yaw_vel_error"] == pytest.approx(0.1, rel=1e-6)
    assert list(s["reward_terms"]) == S.REWARD_NAMES
    assert [v for v in s["reward_terms"].values()] == pytest.approx([0.01 * k for k in range(1, 10)], rel=1e-6)


def test_random_sequence_and_a_window_restart(host):
    """Random buffers for 300 records of 37 envs, resets by the step's own rule and late or outside ones, two windows, restarts in between."""
    rng = np.random.default_rng(5)
    n = 37
    p = Pair(host, n, max_len=60.0)
    for t in range(300):
        p.root[:] = rng.normal(0, 0.3, p.root.shape).astype(np.float32)
        p.root[:, 3:6] = rng.normal(0, 0.1, (n, 3))
        p.root[:, 2] = rng.uniform(0.59, 1.0, n)
        p.root[:, 6] = 1.0
        p.cf[:] = rng.normal(0, 1, p.cf.shape).astype(np.float32) * (rng.random((n, NB, 1)) < 0.0005) * 30
        p.cf[:, 8, 2] = rng.uniform(0, 1600, n)
        p.cf[:, 16, 2] = rng.uniform(0, 1600, n)
        p.rbp[:, (8, 16), 2] = rng.uniform(0, 0.505, (n, 2))
        p.cmd[:] = rng.uniform(-0.6, 1.1, (n, 3))
        p.rew[:] = rng.normal(0, 1, n)
        p.rv[:] = rng.normal(0, 1, (n, 9))
        if t % 40 == 7:
            p.root[rng.integers(0, n), rng.integers(0, 13)] = np.nan
        p.step()
        done = np.nonzero(p.ref.si[K["DWE_ST_CLOSED"]] != 0)[0]
        done = done[rng.random(done.size) < 0.8]             # (some ended envs are reset a few steps late)
        p.reset_done(np.concatenate([done, rng.choice(n, 1) if t % 25 == 3 else []]).astype(np.int64))
        if t == 150:
            p.summary()
            p.ac[:] = 0
            p.ct[:K["DWE_CT_WINDOW"]] = 0
            p.ref.reset_totals()
        if t in (90, 200):
            p.restart(rng.choice(n, 5, replace=False))
    s = p.summary()
    assert s["records"] == 149 and s["record_calls"] == 300
    assert s["episodes"] == sum(s["cause_masks"].values()) > 0 and "none" not in s["cause_masks"]
    assert all(v > 0 for v in s["causes"].values())
    assert s["discarded"] > 0 and s["unreset_steps"] > 0 and s["nonfinite_steps"] > 0


# ---------------------------------------------------------------------------------------------- the kernels' budget
def test_the_new_kernels_use_no_scratch():
    from isaacgymdyros_amd import build
    from test_kernel_resources import resource_usage
    extra = dict(build.SOURCES)["dw_amp_stats.hip"]
    assert "-ffp-contract=off" in extra
    u = resource_usage("dw_amp_stats.hip", extra)
    rec = [r for k, r in u.items() if "dwe_k_record" in k]
    summ = [r for k, r in u.items() if "dwe_k_summarize" in k]
    assert len(rec) == 1 and len(summ) == 1, sorted(u)
    assert rec[0]["ScratchSize"] == 0 and summ[0]["ScratchSize"] == 0, u
    assert rec[0]["LDS Size"] <= 20480, rec          # (eight workgroups per CU)
    assert not any("dw_k_amp" in k for k in u)       # (test_kernel_resources' pattern for the fused step's kernels does not take these)
    assert "dw_amp_stats.h" in build.HEADERS
