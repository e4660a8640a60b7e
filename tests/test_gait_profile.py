"""The gait profile without a GPU (include/dyros_gait.h, isaacgymdyros_amd/csrc/dw_gait.h): the per-env sample --
compiled by g++ from the header the HIP kernel includes (tests/gait_host.cpp) -- against the numpy restatement of tests/gait_profile_ref.py,
every word as an integer; the bins' window labels against the reward's rule; summary()'s derived numbers against float64 numpy on a
hand-built table; the file formats; the cfg checks."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from isaacgymdyros_amd import gait_profile as G
from gait_profile_ref import E, EDGES, F, K, LF, NAN_SPANS, RF, W, Synth, fx, record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 300


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/gait_host.cpp")
    so = str(tmp_path_factory.mktemp("dwgh") / "libdwgh.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, os.path.join(ROOT, "tests", "gait_host.cpp")])
    lib = C.CDLL(so)
    P, I = C.c_void_p, C.c_int
    lib.dwgh_record.argtypes = [I, I, I, I] + [P] * 10
    lib.dwgh_fx.argtypes, lib.dwgh_fx.restype = [C.c_double], C.c_int64
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_record(lib, bufs, bins, min_step, skip, table, ct):
    assert lib.dwgh_record(len(bufs[-1]), bins, min_step, int(skip), *[_p(b) for b in bufs], _p(table), _p(ct)) == 0


def both(lib, syn, bins, min_step, skip, steps=3):
    got, want = np.zeros((bins, W), np.int64), np.zeros((bins, W), np.int64)
    gct, wct = np.zeros(K["DWG_CT_WORDS"], np.int64), np.zeros(K["DWG_CT_WORDS"], np.int64)
    for _ in range(steps):
        bufs = syn.step()
        host_record(lib, bufs, bins, min_step, skip, got, gct)
        record(bufs, bins, min_step, skip, want, wct)
    assert np.array_equal(gct, wct), (gct, wct)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    assert int(gct.sum()) == steps * syn.n and int(got[:, 0].sum()) == int(gct[0])
    return got, gct


# ---------------------------------------------------------------------------------------------- 1. numpy against the g++ build
def test_the_synthetic_buffers_hold_the_cases():
    bufs = Synth(N, 0).step()
    root, dof, cf, es, stacked, reset, progress, tm = bufs
    idx = es.view(np.int32)[:, E["DW_ES_MOCAP_IDX"]]
    assert idx[:len(EDGES)].tolist() == list(EDGES) and idx.min() >= 0 and idx.max() <= 3598
    fz = cf[:, [LF, RF], 2]
    assert (fz < 0).any() and (fz == 1.0).any() and (fz > 1.0).any() and (fz == 0.0).any() and (np.abs(fz) > 2.0 ** 30).sum() == 2
    assert (reset != 0).any() and (reset == 0).sum() > N // 2 and (progress < 5).any() and (progress >= 5).any()
    assert es.view(np.int32)[:, E["DW_ES_PERT_ON"]].any()


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("min_step", [0, 5])
@pytest.mark.parametrize("bins", G.BINS)
def test_record_matches_numpy_as_integers(host, bins, min_step, skip):
    table, ct = both(host, Synth(N, 1000 * bins + 10 * min_step + skip), bins, min_step, skip)
    assert ct[K["DWG_CT_DISCARDED"]] == 0 and ct[K["DWG_CT_SKIPPED_TERMINAL"]] > 0 and ct[K["DWG_CT_RECORDED"]] > N
    assert (ct[K["DWG_CT_SKIPPED_FILTER"]] > 0) == (min_step > 0 or skip)
    assert (table[:, K["DWG_R_PERT"]].sum() == 0) == skip
    # envs 11 and 12 carry sole forces and a torque above the clamp: each adds exactly +-2^46, and 2^46 for the square
    assert table[:, K["DWG_R_FZ"]].max() >= 1 << 45 and table[:, K["DWG_R_FZ"] + 1].min() <= -(1 << 45)
    assert table[:, K["DWG_R_FZ2"]].max() >= 1 << 46 and table[:, K["DWG_R_TORQUE"]].max() >= 1 << 46


@pytest.mark.parametrize("span", sorted(NAN_SPANS))
def test_a_non_finite_word_in_any_span_read_discards_the_env_step(host, span):
    clean, cct = both(host, Synth(N, 7), 72, 0, False, steps=1)
    table, ct = both(host, Synth(N, 7, nan_span=span), 72, 0, False, steps=1)
    bufs = Synth(N, 7).step()
    hit = (bufs[5][0:N:3] == 0).sum()          # every third env is poisoned; those that reset are terminal first
    assert ct[K["DWG_CT_DISCARDED"]] == hit > 0
    assert ct[K["DWG_CT_RECORDED"]] == cct[K["DWG_CT_RECORDED"]] - hit and ct[K["DWG_CT_SKIPPED_TERMINAL"]] == cct[K["DWG_CT_SKIPPED_TERMINAL"]]
    assert table[:, 0].sum() == clean[:, 0].sum() - hit


def test_words_that_are_not_read_discard_nothing(host):
    clean, cct = both(host, Synth(N, 7), 72, 0, False, steps=1)
    table, ct = both(host, Synth(N, 7, unread_nan=True), 72, 0, False, steps=1)
    assert np.array_equal(ct, cct) and np.array_equal(table, clean)


def one_env(fl, fr, idx, tf=(-500.0, -500.0), tm=104.48, paid=0.2, reset=0, progress=9, pert=0):
    root, dof = np.zeros((1, 13), F), np.zeros((1, E["DW_NUM_DOF"], 2), F)
    cf, es, stacked = np.zeros((1, E["DW_NUM_BODIES"], 3), F), np.zeros((1, E["DW_ES_WORDS"]), F), np.zeros((1, 15), F)
    root[0, 2], root[0, 7] = 0.875, 0.5
    dof[0, :12, 0] = np.arange(12) / 8.0
    cf[0, LF, 2], cf[0, RF, 2] = fl, fr
    es[0, E["DW_ES_TARGET_FORCE"]:E["DW_ES_TARGET_FORCE"] + 2] = tf
    es[0, E["DW_ES_TARGET_VEL"]] = 0.25
    es[0, E["DW_ES_TARGET_QPOS"]:E["DW_ES_TARGET_QPOS"] + 12] = 1.0
    es[0, E["DW_ES_ACTION_TORQUE"]:E["DW_ES_ACTION_TORQUE"] + 12] = -np.arange(12) * 0.5
    es.view(np.int32)[0, E["DW_ES_MOCAP_IDX"]], es.view(np.int32)[0, E["DW_ES_PERT_ON"]] = idx, pert
    stacked[0, K["DWG_PAID_COLUMN"]] = paid
    return (root, dof, cf, es, stacked, np.asarray([reset], np.int64), np.asarray([progress], np.int64), np.asarray([tm], F))


def test_one_env_by_hand(host):
    """Every value is exact in float32 and in 2^-16 units, so the expected row is written down, not computed."""
    table, ct = np.zeros((12, W), np.int64), np.zeros(4, np.int64)
    host_record(host, one_env(1.0, 700.5, 300), 12, 0, False, table, ct)          # bin 1 (RSSP): F_z of exactly 1.0 is no contact
    S = 65536
    row = table[1]
    assert ct.tolist() == [1, 0, 0, 0] and not table[[0] + list(range(2, 12))].any()
    assert row[:16].tolist() == [1, S, 700 * S + S // 2, S, int(700.5 ** 2 * S), 500 * S, 500 * S, 499 * S, 200 * S + S // 2, 0, 1, 1, 1,
                                 S * 7 // 8, S // 4, 0]
    assert row[16:28].tolist() == [int(abs(j / 8.0 - 1.0) * S) for j in range(12)] and row[28:40].tolist() == [j * S // 2 for j in range(12)]
    # the same env one row earlier is in DSP, where the rule wants both soles: not predicted, though the kernel's column says paid
    host_record(host, one_env(1.0, 700.5, 299), 12, 0, False, table, ct)
    assert table[0, K["DWG_R_PAID"]] == 1 and table[0, K["DWG_R_PREDICTED"]] == 0
    # the three ways to add nothing, in their order of precedence: terminal before the filters before a NaN
    for kw, word in ((dict(reset=1, progress=0, fl=np.nan), 1), (dict(progress=2, fl=np.nan), 2), (dict(fl=np.nan), 3), (dict(idx=3600), 3),
                     (dict(idx=-1), 3)):
        t2, c2 = np.zeros((12, W), np.int64), np.zeros(4, np.int64)
        args = dict(fl=5.0, fr=5.0, idx=0)
        args.update(kw)
        host_record(host, one_env(**args), 12, 3, False, t2, c2)
        assert not t2.any() and c2.tolist() == [int(i == word) for i in range(4)], kw
    t2, c2 = np.zeros((12, W), np.int64), np.zeros(4, np.int64)
    host_record(host, one_env(5.0, 5.0, 0, pert=1), 12, 0, True, t2, c2)
    assert c2.tolist() == [0, 0, 1, 0]
    host_record(host, one_env(5.0, 5.0, 0, pert=1), 12, 0, False, t2, c2)
    assert c2.tolist() == [1, 0, 1, 0] and t2[0, K["DWG_R_PERT"]] == 1 and t2[0, K["DWG_R_PREDICTED"]] == 1


def test_fixed_point_rounds_to_even_and_clamps(host):
    for v, want in ((0.5 / 65536, 0), (1.5 / 65536, 2), (2.5 / 65536, 2), (-0.5 / 65536, 0), (-1.5 / 65536, -2), (-1.0, -65536), (3.0e9, 1 << 46),
                    (-3.0e9, -(1 << 46)), (2.0 ** 30, 1 << 46), (1e300, 1 << 46), (0.1, 6554)):
        assert host.dwgh_fx(v) == want == int(fx(v)), v


# ---------------------------------------------------------------------------------------------- 2. windows
@pytest.mark.parametrize("bins", G.BINS)
def test_every_bin_lies_in_the_window_of_each_of_its_rows(host, bins):
    def rule(idx):          # dw_oct_post.h:333-335
        DSP = (3300 <= idx < 3600) or (idx < 300) or (1500 <= idx < 2100)
        RSSP, LSSP = 300 <= idx < 1500, 2100 <= idx < 3300
        assert DSP + RSSP + LSSP == 1
        return "DSP" if DSP else ("RSSP" if RSSP else "LSSP")
    width = 3600 // bins
    labels = [G.WINDOWS[w] for w in G.bin_windows(bins)]
    for idx in range(3600):
        assert labels[idx // width] == rule(idx) == G.WINDOWS[host.dwgh_window_of(idx)], idx
    assert host.dwgh_bins_ok(bins) == 1


@pytest.mark.parametrize("bins", [0, 1, 10, 18, 48, 60, 100, 143, 288, 3600, -72, 72.0, "72", True, None])
def test_other_bin_counts_raise(host, bins):
    with pytest.raises(ValueError):
        G.check_bins(bins)
    with pytest.raises(ValueError):
        G.resolve({"bins": bins})
    if isinstance(bins, int):
        assert host.dwgh_bins_ok(int(bins)) == 0
        assert host.dwgh_record(1, int(bins), 0, 0, *[None] * 10) == -1


def test_cfg_spec():
    assert G.resolve(None) is None and G.resolve(False) is None
    assert G.resolve(True) == G.resolve({}) == {"bins": 72, "min_episode_step": 0, "skip_pushes": False}
    assert G.resolve({"bins": 144, "skip_pushes": True}) == {"bins": 144, "min_episode_step": 0, "skip_pushes": True}
    for bad in (1, "on", {"bin": 72}, {"min_episode_step": -1}, {"min_episode_step": 1.5}, {"skip_pushes": 1}, [72]):
        with pytest.raises(ValueError):
            G.resolve(bad)
    from isaacgymdyros_amd.config import default_cfg, validate_cfg
    cfg = default_cfg(64, "cpu")
    assert "gait_profile" not in cfg["sim"]["mi355"]          # (off by default)
    cfg["sim"]["mi355"]["gait_profile"] = {"bins": 36}
    validate_cfg(cfg)
    cfg["sim"]["mi355"]["gait_profile"] = {"bins": 35}
    with pytest.raises(ValueError):
        validate_cfg(cfg)


# ---------------------------------------------------------------------------------------------- 3. the summary
def hand_table(bins=12):
    """A table whose rows differ, with one empty bin; built from integers so that float64 restates it without rounding questions."""
    r = np.random.default_rng(5)
    t = np.zeros((bins, W), np.int64)
    n = r.integers(1, 2000, bins)
    n[4] = 0
    for w in range(1, W):
        t[:, w] = r.integers(-(1 << 30), 1 << 30, bins) * (n > 0)
    for w in (9, 10, 11, 12, 15):
        t[:, w] = r.integers(0, n + 1)
    fz = t[:, 1:3] / 65536.0 / np.maximum(n, 1)[:, None]
    t[:, 3:5] = np.rint((fz ** 2 + r.uniform(0.0, 50.0, (bins, 2))) * np.maximum(n, 1)[:, None] * 65536.0) * (n > 0)[:, None]
    t[:, 0] = n
    return t


def test_summary_against_float64_numpy():
    t = hand_table()
    ct = [int(t[:, 0].sum()), 11, 22, 33]
    mocap = np.arange(3600 * 36, dtype=np.float32).reshape(3600, 36)
    s = G.fold(t, ct, mocap)
    n = t[:, 0].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = t.astype(np.float64) / 65536.0 / n[:, None]
        fr = t.astype(np.float64) / n[:, None]
        assert np.array_equal(s["count"], t[:, 0]) and s["bins"] == 12 and np.array_equal(s["table"], t)
        assert np.array_equal(s["fz"], m[:, 1:3], equal_nan=True) and np.array_equal(s["expected_fz"], m[:, 5:7], equal_nan=True)
        assert np.array_equal(s["force_err"], m[:, 7:9], equal_nan=True) and np.array_equal(s["contact_fraction"], fr[:, 9:11], equal_nan=True)
        assert np.array_equal(s["paid_fraction"], fr[:, 11], equal_nan=True) and np.array_equal(s["paid_predicted_fraction"], fr[:, 12], equal_nan=True)
        assert np.array_equal(s["root_z"], m[:, 13], equal_nan=True) and np.array_equal(s["vel_err"], m[:, 14], equal_nan=True)
        assert np.array_equal(s["push_fraction"], fr[:, 15], equal_nan=True)
        assert np.array_equal(s["joint_err"], m[:, 16:28], equal_nan=True) and np.array_equal(s["torque_abs"], m[:, 28:40], equal_nan=True)
        std = np.sqrt(np.maximum(m[:, 3:5] - m[:, 1:3] ** 2, 0.0))
    assert np.array_equal(s["fz_std"], std, equal_nan=True) and (s["fz_std"][n > 0] > 0).all()
    assert np.isnan(s["fz"][4]).all() and np.isnan(s["paid_fraction"][4]) and not np.isnan(np.delete(s["fz"], 4, axis=0)).any()
    assert s["phase"].tolist() == [(b + 0.5) / 12 for b in range(12)]
    # 12 bins of 300 rows: [0, 300) DSP, [300, 1500) RSSP, [1500, 2100) DSP, [2100, 3300) LSSP, [3300, 3600) DSP
    assert s["window"] == ["DSP"] + ["RSSP"] * 4 + ["DSP"] * 2 + ["LSSP"] * 4 + ["DSP"]
    members = {"DSP": [0, 5, 6, 11], "RSSP": [1, 2, 3, 4], "LSSP": [7, 8, 9, 10]}
    for name, rows in members.items():
        w, tot = s["windows"][name], t[rows].sum(axis=0).astype(np.float64)
        assert w["count"] == int(tot[0]) > 0
        assert np.array_equal(w["fz"], tot[1:3] / 65536.0 / tot[0]) and np.array_equal(w["force_err"], tot[7:9] / 65536.0 / tot[0])
        assert w["paid_fraction"] == tot[11] / tot[0] and w["paid_predicted_fraction"] == tot[12] / tot[0]
        assert np.array_equal(w["fz_std"], np.sqrt(np.maximum(tot[3:5] / 65536.0 / tot[0] - (tot[1:3] / 65536.0 / tot[0]) ** 2, 0.0)))
        assert np.array_equal(w["joint_err"], tot[16:28] / 65536.0 / tot[0])
        assert np.array_equal(w["mocap_force"], s["mocap_force"][rows].mean(axis=0))
    assert s["duty_factor"] == [t[:, 9].sum() / t[:, 0].sum(), t[:, 10].sum() / t[:, 0].sum()]
    assert (s["recorded"], s["skipped_terminal"], s["skipped_filter"], s["discarded"]) == tuple(ct)
    # mocap_force: the mean of columns 34 / 35 over the bin's 300 rows
    want = np.stack([mocap[b * 300:(b + 1) * 300, 34:36].astype(np.float64).mean(axis=0) for b in range(12)])
    assert np.array_equal(s["mocap_force"], want)
    assert "DSP" in G.format_table(s) and "RSSP paid" in G.format_line(s)


def test_packaged_mocap_force_columns():
    """The packaged table's force columns are zero for the swing foot in the single-support windows: left (34) in RSSP, right (35) in LSSP."""
    f = G.mocap_force(12)
    assert f.shape == (12, 2) and (f <= 0).all()
    assert (f[2:4, 0] == 0).all() and (f[2:4, 1] < -1000).all() and (f[8:10, 1] == 0).all() and (f[8:10, 0] < -1000).all()


def test_files_round_trip(tmp_path):
    s = G.fold(hand_table(24), [1, 2, 3, 4])
    G.write_npz(str(tmp_path / "g.npz"), s)
    z = np.load(str(tmp_path / "g.npz"))
    for k, v in G.flat(s).items():
        assert np.array_equal(z[k], v, equal_nan=v.dtype.kind == "f"), k
    assert z["windows_fz"].shape == (3, 2) and z["table"].dtype == np.int64 and z["window"].tolist() == s["window"]
    path = G.write_txt(str(tmp_path / "txt"), s)
    lines = open(path).read().splitlines()
    assert len(lines) == 1 + 24 and all(len(x.split("\t")) == 3 + len(G.TXT_COLUMNS) for x in lines)
    back = G.read_txt(path)
    eq = lambda a, b: np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)          # noqa: E731
    assert back["bin"] == list(range(24)) and back["window"] == s["window"] and back["count"] == s["count"].tolist()
    assert eq(back["phase"], s["phase"]) and eq(back["fz_l"], s["fz"][:, 0]) and eq(back["fz_std_r"], s["fz_std"][:, 1])
    assert eq(back["paid_fraction"], s["paid_fraction"]) and eq(back["mocap_force_r"], s["mocap_force"][:, 1])
    assert eq(back["joint_err_11"], s["joint_err"][:, 11]) and eq(back["torque_abs_0"], s["torque_abs"][:, 0])
