"""The run trace without a GPU (include/dyros_trace.h, isaacgymdyros_amd/csrc/dw_trace.h): the row assembly and the slot
state -- compiled by g++ from the same header the HIP kernels include (tests/trace_host.cpp) -- against the numpy restatement of
tests/run_trace_ref.py on synthetic buffers, bit for bit; the row layout, the derived prototypes and the cfg key."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from isaacgymdyros_amd import abi, build
from isaacgymdyros_amd import run_trace as T
from run_trace_ref import NB, Synth, TraceRef, non_foot_max

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, E = T.K, abi.K
N, ML = 37, 9.0          # a short episode so that time limits fall inside a test: n1 >= 8


def test_row_layout_tiles_the_row():
    spans = sorted((K[k], K["DWT_LEN_" + k[len("DWT_CH_"):]]) for k in K if k.startswith("DWT_CH_"))
    assert len(spans) == len(T.CHANNELS) == sum(k.startswith("DWT_LEN_") for k in K)
    at = 0
    for off, n in spans:
        assert off == at and n >= 1, (off, at)          # no gap, no overlap
        at += n
    assert at == K["DWT_ROW_WORDS"] and K["DWT_ROW_WORDS"] % 4 == 0
    assert sorted((o, int(np.prod(s, dtype=np.int64))) for o, s, _k in T.CHANNELS.values()) == spans
    assert [n for n, (_o, _s, kind) in T.CHANNELS.items() if kind == "i"] == ["seen", "epi_step", "flags", "nan_resets"]
    lens = {n: int(np.prod(s, dtype=np.int64)) for n, (_o, s, _k) in T.CHANNELS.items()}
    assert (lens["root_states"], lens["dof_pos"], lens["dof_vel"], lens["qpos_noise"], lens["target_data_qpos"], lens["actions"],
            lens["action_torque"], lens["foot_forces"], lens["stacked_rewards"]) == (13, 33, 33, 33, 33, 13, 12, 6, 15)
    assert sorted(T.FLAGS.values()) == [1, 2, 4, 8, 16]


def test_ctypes_prototypes_match_the_header():
    import test_cbind as TC
    TC.test_ctypes_prototypes_match_the_header("dyros_trace.h", "dwt_", "run_trace", C.CDLL(build.build()))


def test_validate_cfg_checks_the_switch():
    from isaacgymdyros_amd.config import default_cfg, validate_cfg
    cfg = default_cfg(64, "cpu")
    validate_cfg(cfg)                                            # off by default
    assert "run_trace" not in cfg["sim"]["mi355"]
    good = {"env_ids": [5, 0, 63], "depth": 16, "hold": "fall"}
    for spec in (good, dict(good, env_ids=64), dict(good, hold="never"), dict(good, hold="reset"), {"env_ids": 64, "depth": 512}):
        cfg["sim"]["mi355"]["run_trace"] = spec
        validate_cfg(cfg)
    for bad, what in ((dict(good, env_ids=[0, 64]), "env_ids"), (dict(good, env_ids=[-1]), "env_ids"), (dict(good, env_ids=65), "env_ids"),
                      (dict(good, env_ids=[3, 3]), "repeats"), (dict(good, env_ids=[]), "env_ids"), (dict(good, depth=0), "depth"),
                      (dict(good, depth=-4), "depth"), (dict(good, hold="always"), "hold"), (dict(good, bogus=1), "bogus"),
                      (dict(good, env_ids=64, depth=(1 << 30) // (64 * T.ROW_BYTES) + 1), "1 GiB"), (True, "run_trace")):
        cfg["sim"]["mi355"]["run_trace"] = bad
        with pytest.raises(ValueError, match=what):
            validate_cfg(cfg)
    cfg["sim"]["mi355"]["run_trace"] = dict(good, env_ids=64, depth=(1 << 30) // (64 * T.ROW_BYTES))          # exactly at the limit
    validate_cfg(cfg)
    assert 64 * 512 * T.ROW_BYTES == 27262976                    # the default use: about 27 MB


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/trace_host.cpp")
    so = str(tmp_path_factory.mktemp("dwth") / "libdwth.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, os.path.join(ROOT, "tests", "trace_host.cpp")])
    lib = C.CDLL(so)
    P, I, F = C.c_void_p, C.c_int32, C.c_float
    lib.dwth_record.argtypes = [I, I, I, I] + [P] * 9 + [F, P, P]
    lib.dwth_arm.argtypes = [I, I, P, I, P, P, P]
    lib.dwth_gather.argtypes = [I, I, P, I, P, P, P, P]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Pair:
    """The g++ build and the numpy restatement, driven with the same buffers and compared after every call."""

    def __init__(self, host, env_ids, depth, hold, n=N, max_len=ML, seed=0):
        self.h, self.n, self.k, self.depth, self.ml = host, n, len(env_ids), depth, max_len
        self.ref = TraceRef(n, env_ids, depth, hold, max_len)
        self.ring = np.zeros_like(self.ref.ring)
        self.ss = np.zeros_like(self.ref.ss)
        self.syn = Synth(n, max_len, seed)
        self.arm()

    def arm(self, ids=None):
        a = None if ids is None else np.ascontiguousarray(ids, np.int32)
        self.h.dwth_arm(self.n, self.k, None if a is None else _p(a), 0 if a is None else a.size, _p(self.syn.count), _p(self.ref.env_slot), _p(self.ss))
        self.ref.arm(self.syn.count, ids)
        self.check()

    def record(self, bufs):
        root, dof, cf, es, rew, stacked, reset, timeout = [np.ascontiguousarray(b) for b in bufs]
        self.h.dwth_record(self.n, self.k, self.depth, self.ref.hold, _p(self.ref.slot_env), _p(root), _p(dof), _p(cf), _p(es), _p(rew), _p(stacked),
                           _p(reset), _p(timeout), self.ml, _p(self.ss), _p(self.ring))
        self.ref.record(root, dof, cf, es, rew, stacked, reset, timeout)
        self.check()

    def step(self, **kw):
        self.record(self.syn.step(**kw))

    def check(self):
        assert np.array_equal(self.ss, self.ref.ss), np.nonzero(self.ss != self.ref.ss)
        assert np.array_equal(self.ring, self.ref.ring), np.nonzero(self.ring != self.ref.ring)

    def gather(self, slots):
        ids = np.ascontiguousarray(slots, np.int32)
        out = np.full((len(slots), self.depth, K["DWT_ROW_WORDS"]), 0xdeadbeef, np.uint32)
        nr = np.full(len(slots), -7, np.int32)
        self.h.dwth_gather(self.k, self.depth, _p(ids), len(slots), _p(self.ss), _p(self.ring), _p(out), _p(nr))
        want, want_nr = self.ref.gather(slots)
        assert np.array_equal(nr, want_nr) and np.array_equal(out, want)
        return T.decode(out), nr


def env_ids_of(k, seed=1):
    return np.random.default_rng(seed).permutation(N)[:k].tolist()


@pytest.mark.parametrize("hold", ["never", "fall", "reset"])
@pytest.mark.parametrize("depth", [1, 4, 7])
@pytest.mark.parametrize("k", [1, 3, 4, 5, 37])
def test_record_matches_numpy_bit_for_bit(host, k, depth, hold):
    p = Pair(host, env_ids_of(k, seed=k), depth, hold, seed=100 * k + depth)
    for t in range(3 * depth + 2):
        p.step()
        if hold != "never" and t == 2 * depth:                   # release every other slot: exactly those record again
            held0 = p.ss[K["DWT_SS_HELD"]].copy()
            sub = p.ref.slot_env[::2]
            p.arm(sub)
            assert not p.ss[K["DWT_SS_HELD"], ::2].any() and np.array_equal(p.ss[K["DWT_SS_HELD"], 1::2], held0[1::2])
    if hold == "never":
        assert (p.ss[K["DWT_SS_CURSOR"]] == 3 * depth + 2).all() and not p.ss[K["DWT_SS_HELD"]].any()          # every ring wrapped
    out, nr = p.gather(list(range(k)))
    assert (out["pad"] == 0).all()


def test_falls_time_limits_and_both_occur(host):
    """The scripted resets of one long run hold all three kinds of step: a fall, a time limit, and both in one record."""
    p = Pair(host, list(range(N)), 4, "never", seed=3)
    kinds = np.zeros(3, np.int64)
    for _ in range(40):
        p.step()
        fl = p.gather(list(range(N)))[0]["flags"]
        last = np.minimum(p.ss[K["DWT_SS_CURSOR"]], 4) - 1
        r, tl = fl["reset"][np.arange(N), last], fl["time_limit"][np.arange(N), last]
        kinds += [int((r & ~tl).any()), int((r & tl).any()), int((r & ~tl).any() and (r & tl).any())]
    assert (kinds > 0).all(), kinds
    assert p.ss[K["DWT_SS_FALLS"]].sum() > 0


@pytest.mark.parametrize("hold", ["fall", "reset"])
def test_a_held_ring_is_frozen_while_seen_advances(host, hold):
    p = Pair(host, env_ids_of(5, seed=9), 4, hold, seed=11)
    for _ in range(30):                                          # (0.15 per step, and a time limit every 8: every slot resets)
        p.step()
    held = p.ss[K["DWT_SS_HELD"]] != 0
    assert held.any() and (held.all() or hold == "fall")
    ring0, ss0 = p.ring.copy(), p.ss.copy()
    for _ in range(6):
        p.step()
    h = np.nonzero(held)[0]
    assert np.array_equal(p.ring[h], ring0[h])
    assert np.array_equal(p.ss[K["DWT_SS_SEEN"], h], ss0[K["DWT_SS_SEEN"], h] + 6)
    for w in ("CURSOR", "HELD", "N", "FALLS"):
        assert np.array_equal(p.ss[K["DWT_SS_" + w], h], ss0[K["DWT_SS_" + w], h])
    # the frozen ring ends with the terminating step: reset set, and for hold "fall" no time limit
    out, nr = p.gather(h.tolist())
    last = nr - 1
    fl = out["flags"]
    assert fl["reset"][np.arange(len(h)), last].all()
    if hold == "fall":
        assert not fl["time_limit"][np.arange(len(h)), last].any()
    # arm on a subset resumes exactly those slots, their episode count restarting from progress_buf
    sub = p.ref.slot_env[h[:1]]
    p.arm(sub)
    assert p.ss[K["DWT_SS_HELD"], h[0]] == 0 and p.ss[K["DWT_SS_CURSOR"], h[0]] == 0 and p.ss[K["DWT_SS_SEEN"], h[0]] == 0
    assert p.ss[K["DWT_SS_N"], h[0]] == p.syn.count[sub[0]]
    p.arm(np.array([N + 5, -3], np.int32))                       # ids out of range, and below an env that is not traced: ignored
    untraced = [e for e in range(N) if e not in p.ref.slot_env.tolist()][:2]
    p.arm(untraced)
    ss1 = p.ss.copy()
    p.step(fall_p=0.0)
    assert p.ss[K["DWT_SS_CURSOR"], h[0]] == 1
    assert np.array_equal(p.ss[K["DWT_SS_CURSOR"], h[1:]], ss1[K["DWT_SS_CURSOR"], h[1:]])


def test_non_foot_maximum_ties_and_zero_row(host):
    p = Pair(host, [0, 1, 2, 3], 2, "never")
    bufs = list(p.syn.step(fall_p=0.0))
    cf = np.zeros((N, NB, 3), np.float32)
    cf[0, 30] = (0.0, 3.0, 4.0)                                  # two equal maxima: the lowest row wins
    cf[0, 11] = (3.0, 4.0, 0.0)
    cf[0, 8] = (0.0, 0.0, 900.0)                                 # the soles never count
    cf[0, 16] = (0.0, 0.0, 800.0)
    cf[2, 37] = (0.0, 0.0, -2.0)                                 # the last body
    cf[3, 8] = (1.0, 2.0, 3.0)                                   # only a sole loaded: the others' maximum is 0 at row 0
    bufs[2] = cf
    p.record(bufs)
    out, _ = p.gather([0, 1, 2, 3])
    assert out["non_foot_max"][:, 0].tolist() == [5.0, 0.0, 2.0, 0.0]
    assert out["non_foot_body"][:, 0].tolist() == [11.0, 0.0, 37.0, 0.0]
    assert out["foot_forces"][0, 0].tolist() == [[0.0, 0.0, 900.0], [0.0, 0.0, 800.0]] and out["foot_forces"][3, 0, 0].tolist() == [1.0, 2.0, 3.0]
    v, g = non_foot_max(cf[:1])
    assert (float(v[0]), int(g[0])) == (5.0, 11)


@pytest.mark.parametrize("records", [0, 2, 5, 6, 13])
def test_gather_is_chronological(host, records):
    """cursor < depth, == depth and > depth (once and twice around): oldest first, unused rows zero."""
    depth = 5
    p = Pair(host, env_ids_of(3, seed=2), depth, "never", seed=records)
    for _ in range(records):
        p.step()
    out, nr = p.gather([2, 0, 1, 7, -1])                         # (a slot id out of range gives zero rows)
    assert nr.tolist() == [min(records, depth)] * 3 + [0, 0]
    for i in range(3):
        assert out["seen"][i].tolist() == list(range(records - nr[i] + 1, records + 1)) + [0] * (depth - nr[i])
    assert not out["seen"][3:].any() and not out["root_states"][3:].any()
    used = np.arange(depth)[None, :] < nr[:, None]
    assert not out["root_states"][~used].any() and not out["flags"]["bits"][~used].any()


def test_channels_hold_the_buffers_they_name(host):
    """One record, read back through CHANNELS, against the source buffers directly (dof_state de-interleaved)."""
    ids = env_ids_of(5, seed=4)
    p = Pair(host, ids, 3, "never", seed=8)
    p.syn.count[:] = np.arange(N) % 5                            # an explicit restart picks the count up from progress_buf
    p.arm()
    root, dof, cf, es, rew, stacked, reset, timeout = bufs = p.syn.step()
    p.record(bufs)
    out, _ = p.gather(list(range(5)))
    r = {k: v[:, 0] for k, v in out.items() if k != "flags"}
    assert np.array_equal(r["root_states"], root[ids]) and np.array_equal(r["dof_pos"], dof[ids, :, 0]) and np.array_equal(r["dof_vel"], dof[ids, :, 1])
    for name in ("qpos_noise", "target_data_qpos", "actions", "action_torque", "target_data_force", "target_vel"):
        assert np.array_equal(r[name], abi.es_view(es, name)[ids]), name
    for name in ("magnitude", "phase"):
        assert np.array_equal(r[name], abi.es_view(es, name)[ids])
    assert np.array_equal(r["time"], abi.es_view(es, "time")[ids, 0])
    assert np.array_equal(r["rew_buf"], rew[ids]) and np.array_equal(r["stacked_rewards"], stacked[ids])
    assert np.array_equal(r["nan_resets"], abi.es_view(es, "nan_resets")[ids])
    assert r["epi_step"].tolist() == [(e % 5) + 1 for e in ids] and r["seen"].tolist() == [1] * 5
    fl = {k: v[:, 0] for k, v in out["flags"].items()}
    assert np.array_equal(fl["reset"], reset[ids] != 0) and np.array_equal(fl["timeout"], timeout[ids] != 0)
    assert np.array_equal(fl["pert_on"], abi.es_view(es, "pert_on")[ids] != 0)
    assert np.array_equal(fl["perturb_start"], abi.es_view(es, "perturb_start")[ids, 0] != 0)
    assert np.array_equal(fl["time_limit"], np.array([(e % 5) + 1 >= ML - 1 for e in ids]))


def test_the_cursor_folds_before_it_wraps(host):
    """A count that reaches DWT_CURSOR_FOLD continues from depth + cursor % depth: the next row, the row count and the order stay right
    (depth 7 does not divide 2^32, so a plain wrap would jump)."""
    depth = 7
    p = Pair(host, [3, 9], depth, "never", seed=21)
    for _ in range(depth + 2):
        p.step(fall_p=0.0)
    start = K["DWT_CURSOR_FOLD"] - 3
    start -= (start - int(p.ss[K["DWT_SS_CURSOR"], 0])) % depth          # (a count with the same next row as the real one)
    p.ss[K["DWT_SS_CURSOR"], :] = p.ref.ss[K["DWT_SS_CURSOR"], :] = start
    for t in range(12):
        p.step(fall_p=0.0)
        out, nr = p.gather([0, 1])
        assert nr.tolist() == [depth, depth]
        assert (np.diff(out["seen"], axis=1) == 1).all() and (out["seen"][:, -1] == depth + 3 + t).all()
    cur = p.ss[K["DWT_SS_CURSOR"]]
    assert (cur < 3 * depth).all() and (cur >= depth).all() and (cur % depth == (start + 12) % depth).all()


def _read_like(p, slots):
    """What RunTrace.read returns, from the g++ build's ring."""
    out, nr = p.gather(slots)
    out.update(rows=nr.astype(np.int64), env_ids=p.ref.slot_env[slots].astype(np.int64), held=p.ss[K["DWT_SS_HELD"], slots] != 0,
               cursor=p.ss[K["DWT_SS_CURSOR"], slots].astype(np.int64), falls=p.ss[K["DWT_SS_FALLS"], slots].astype(np.int64))
    return out


def test_episodes_split_at_the_reset_flags(host):
    """Several episodes in one ring: pieces end with a flagged row, a running episode is the trailing piece, a ring that ends with a flagged
    row has no trailing piece, and the pieces put together are the ring."""
    depth = 24
    p = Pair(host, [5, 6, 7], depth, "never", seed=31)
    script = {4: [1, 0, 0], 5: [1, 1, 0], 11: [1, 0, 0], 29: [0, 1, 0]}          # step -> which of the three envs reset
    for t in range(30):
        bufs = list(p.syn.step(fall_p=0.0))
        reset = np.zeros(N, np.int64)
        reset[[5, 6, 7]] = script.get(t, [0, 0, 0])
        bufs[6] = reset
        p.record(bufs)
    r = _read_like(p, [0, 1, 2])
    # rows 0..23 are steps 6..29: env 5 reset at step 11 (row 5), env 6 at 29 (the last row), env 7 never
    for i in range(3):
        one = T.cut(r, i)
        eps = T.split_episodes(one)
        assert sum(len(e["seen"]) for e in eps) == depth
        assert np.array_equal(np.concatenate([e["root_states"] for e in eps]), one["root_states"])
        for e in eps[:-1]:
            assert e["flags"]["reset"][-1] and not e["flags"]["reset"][:-1].any()
        assert not eps[-1]["flags"]["reset"][:-1].any()
    lens = [[len(e["seen"]) for e in T.split_episodes(T.cut(r, i))] for i in range(3)]
    assert lens == [[6, 18], [24], [24]], lens          # env 5: rows 0..5 end at step 11, then a running piece; env 6: one piece ending flagged
    assert T.split_episodes(T.cut(r, 1))[0]["flags"]["reset"][-1] and not T.split_episodes(T.cut(r, 2))[0]["flags"]["reset"].any()
    fresh = Pair(host, [5], depth, "never")
    assert T.split_episodes(T.cut(_read_like(fresh, [0]), 0)) == []


def test_export_txt_and_npz_round_trip(host, tmp_path):
    depth = 6
    p = Pair(host, [2, 30], depth, "never", seed=41)
    for _ in range(4):
        p.step()
    one = T.cut(_read_like(p, [0, 1]), 1)
    paths = T.write_txt(str(tmp_path / "txt"), one)
    names = sorted(os.path.basename(q) for q in paths)
    assert names == sorted("%s_env30.txt" % n for n in list(T.flat(one)) if isinstance(T.flat(one)[n], np.ndarray))
    assert "dof_pos_env30.txt" in names and "flag_reset_env30.txt" in names and "pad_env30.txt" not in names
    for q in paths:
        name = os.path.basename(q)[:-len("_env30.txt")]
        lines = open(q).read().split("\n")
        assert lines[-1] == "" and len(lines) == 4 + 1          # one line per step
        got = np.array([[float(x) for x in ln.split("\t")] for ln in lines[:-1]])
        src = T.flat(one)[name]
        assert np.array_equal(got.astype(src.dtype).reshape(src.shape), src), name          # (str(float32) round-trips)
    T.write_npz(str(tmp_path / "one.npz"), one)
    z = np.load(tmp_path / "one.npz")
    assert int(z["env_id"]) == 30 and z["foot_forces"].shape == (4, 2, 3) and np.array_equal(z["action_torque"], one["action_torque"])
    for flag, bit in T.FLAGS.items():
        assert np.array_equal(z["flag_" + flag], (z["flags"] & bit) != 0)


def test_an_empty_spec_is_the_default_trace(monkeypatch):
    import types
    from isaacgymdyros_amd import gait_profile, recorders, run_trace
    from isaacgymdyros_amd.config import default_cfg, validate_cfg
    cfg = default_cfg(64, "cpu")
    cfg["sim"]["mi355"]["run_trace"] = {}          # 64 envs, 512 steps, hold "fall": on, as DyrosDynamicWalk reads it too
    validate_cfg(cfg)
    # what DyrosDynamicWalk attaches is recorders.attach's decision: {} and True switch a recorder on (with that spec), None and False off
    monkeypatch.setattr(run_trace, "RunTrace", lambda env, spec: ("run_trace", spec))
    monkeypatch.setattr(gait_profile, "GaitProfile", lambda env, spec: ("gait_profile", spec))
    for key in ("run_trace", "gait_profile"):
        for spec, on in (({}, True), (True, True), (None, False), (False, False)):
            assert recorders.is_on(spec) is on
            env = types.SimpleNamespace(extras={})
            recorders.attach(env, {key: spec})
            assert getattr(env, key) == ((key, spec) if on else None)
            assert all(getattr(env, other) is None for other, _, _ in recorders.WALK if other != key)
    env = types.SimpleNamespace(extras={})
    recorders.attach(env, {})
    assert all(getattr(env, name) is None for name, _, _ in recorders.WALK)
