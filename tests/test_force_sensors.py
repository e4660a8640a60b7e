"""The foot force-torque sensors without a GPU (include/dyros_sensors.h, isaacgymdyros_amd/csrc/dw_sensors.h): the
header, the Python binding and the built library agree; refusals; the kernel's resources; known answers of the float64 restatement
(tests/force_sensors_ref.py) and of the per-env arithmetic compiled by g++ from the header the HIP kernel includes
(tests/force_sensors_host.cpp); the g++ build against the restatement under its measured tolerance; the restatement against the CPU
oracle's own foot forces; the cfg spec."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import body_states_ref as BR
import force_sensors_ref as R
from isaacgymdyros_amd import abi, body_states as B, build, cbind
from isaacgymdyros_amd import force_sensors as FS
from isaacgymdyros_amd.model import load_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dw_sensors.hip"
N = 67
F = np.float32
K = FS.K


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def c_sensors(sensors):
    return FS.sensor_array([dict(s, pos=s.get("pos", [0, 0, -0.09]), quat=s.get("quat", [0, 0, 0, 1]), world_frame=s.get("world_frame", False))
                            for s in sensors])


# ---------------------------------------------------------------------------------------------- 1. the ABI
def declared():
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dyros_sensors.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dwf_[a-z_0-9]+)\s*\(", src)))


@pytest.fixture(scope="module")
def api():
    return cbind.declare(C.CDLL(build.build()), "dyros_sensors.h", "dwf_")


def test_header_python_and_library_agree(api):
    assert declared() == sorted("dwf_" + n for n in FS.EXPORTS) == ["dwf_abi_version", "dwf_last_error", "dwf_refresh"]
    assert dict(build.SOURCES)[SRC] == ["-ffp-contract=off"] and "dw_sensors.h" in build.HEADERS
    lib = C.CDLL(build.build())
    for fn in declared():
        assert hasattr(lib, fn), fn
    assert lib.dwf_abi_version() == K["DWF_ABI_VERSION"] == 1
    assert api["refresh"].argtypes == [C.c_int32] + [C.c_void_p] * 4 + [C.POINTER(FS.DwfModel), C.POINTER(FS.DwfSensor), C.c_int32] + [C.c_void_p] * 5
    assert api["refresh"].restype is C.c_int and api["last_error"].restype is C.c_char_p
    # the record's layout is dyros_walk.h's; the chain constants are dyros_bodies.h's
    assert (K["DWF_ES_WORDS"], K["DWF_ES_WARM"], K["DWF_NUM_CORNERS"]) == (abi.K["DW_ES_WORDS"], abi.K["DW_ES_WARM"], abi.K["DW_NUM_FOOT_PTS"])
    assert K["DWF_ES_WARM"] * 4 == 1376 and K["DWF_ES_WORDS"] * 4 == 1488 and K["DWF_ES_WARM"] % 4 == 0 and K["DWF_WARM_WORDS"] == 24
    assert K["DWF_DOF_ROW"] == 2 * B.K["DWB_NUM_DOF"] and K["DWF_GROUP"] == 16 and K["DWF_MAX_SENSORS"] == 8
    assert (K["DWF_SENSOR_WORDS"], K["DWF_COP_WORDS"], K["DWF_ZMP_WORDS"], K["DWF_CORNER_WORDS"]) == (6, 4, 4, 6)
    assert C.sizeof(FS.DwfModel) == 4 * (2 + 24 + 1) and C.sizeof(FS.DwfSensor) == 4 * 9
    # the kernel's argument block: five input pointers and n, the model, eight sensors, ns, four output pointers -- within HIP's 4 KB
    assert 8 * 5 + C.sizeof(FS.DwfModel) + 8 * C.sizeof(FS.DwfSensor) + 8 + 8 * 4 <= 4096
    m = FS.model_struct(load_model(), 0.002)
    assert list(m.foot_mv) == [6, 12] and m.inv_dt == float(F(1) / F(0.002)) == float(R.INV_DT)
    assert np.array_equal(np.ctypeslib.as_array(m.foot_pos).astype(F), R.FOOT_POS.astype(F))


def test_refusals_happen_before_any_launch(api):
    """Every buffer is NULL or a host address here: a launch would fault, a refusal returns -1 with its message."""
    one, m = C.c_void_p(16), FS.model_struct(load_model(), 0.002)
    two = c_sensors(R.DEFAULT_SENSORS)

    def model(**kw):
        b = FS.model_struct(load_model(), 0.002)
        for k, v in kw.items():
            if k == "foot_mv":
                b.foot_mv[1] = v
            else:
                setattr(b, k, v)
        return b

    def sens(**kw):
        a = c_sensors(R.DEFAULT_SENSORS)
        for k, v in kw.items():
            if k == "quat":
                for i in range(4):
                    a[1].quat[i] = v[i]
            else:
                setattr(a[1], k, v)
        return a
    nine = (FS.DwfSensor * 9)()
    for args, msg in (((0, one, one, one, one, m, two, 2, one, one, one, one, None), b"num_envs"),
                      ((8, None, one, one, one, m, two, 2, one, one, one, one, None), b"a buffer is missing"),
                      ((8, one, None, one, one, m, two, 2, one, one, one, one, None), b"a buffer is missing"),
                      ((8, one, one, None, one, m, two, 2, one, one, one, one, None), b"a buffer is missing"),
                      ((8, one, one, one, None, m, two, 2, one, one, one, one, None), b"a buffer is missing"),
                      ((8, one, one, one, one, None, two, 2, one, one, one, one, None), b"the model is missing"),
                      ((8, one, one, one, one, m, None, 2, one, one, one, one, None), b"the sensor array is missing"),
                      ((8, one, one, one, one, m, nine, 9, one, one, one, one, None), b"ns must be in 0..8"),
                      ((8, one, one, one, one, m, two, -1, one, one, one, one, None), b"ns must be in 0..8"),
                      ((8, one, one, one, one, m, sens(foot=2), 2, one, one, one, one, None), b"foot is outside 0..1"),
                      ((8, one, one, one, one, m, sens(foot=-1), 2, one, one, one, one, None), b"foot is outside 0..1"),
                      ((8, one, one, one, one, m, sens(quat=(0, 0, 0, 1.02)), 2, one, one, one, one, None), b"norm outside"),
                      ((8, one, one, one, one, m, sens(quat=(0, 0, 0, 0.98)), 2, one, one, one, one, None), b"norm outside"),
                      ((8, one, one, one, one, m, sens(quat=(0, float("nan"), 0, 1)), 2, one, one, one, one, None), b"norm outside"),
                      ((8, one, one, one, one, model(inv_dt=float("inf")), two, 2, one, one, one, one, None), b"inv_dt is not finite"),
                      ((8, one, one, one, one, model(inv_dt=float("nan")), two, 2, one, one, one, one, None), b"inv_dt is not finite"),
                      ((8, one, one, one, one, model(foot_mv=13), two, 2, one, one, one, one, None), b"foot_mv is outside 1..12"),
                      ((8, one, one, one, one, m, two, 2, None, one, one, one, None), b"exactly when ns > 0"),
                      ((8, one, one, one, one, m, None, 0, one, one, one, one, None), b"exactly when ns > 0"),
                      ((8, one, one, one, one, m, None, 0, None, None, None, None, None), b"must be given"),
                      ((8, C.c_void_p(4), one, one, one, m, two, 2, one, one, one, one, None), b"table must be 16-byte aligned"),
                      ((8, one, one, one, C.c_void_p(8), m, two, 2, one, one, one, one, None), b"env_state must be 16-byte aligned")):
        assert api["refresh"](*args) == -1 and msg in api["last_error"](), (args, api["last_error"]())


# ---------------------------------------------------------------------------------------------- 2. the kernel's resources
def test_kernel_uses_no_scratch_and_fits_the_lds():
    extra = dict(build.SOURCES)[SRC]
    cmd = [build.hipcc()] + build.FLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(build.CSRC, SRC)]
    remarks = subprocess.run(cmd, cwd=build.CSRC, capture_output=True, text=True, check=True).stderr
    names = re.findall(r"remark: Function Name: (\S+)", remarks)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)]
    assert len(names) == 1 and len(scratch) == len(lds) == 1
    assert "dwf_k_refresh" in names[0] and scratch[0] == 0 and lds[0] <= 65536, (names, scratch, lds)


# ---------------------------------------------------------------------------------------------- 3. the g++ build
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/force_sensors_host.cpp")
    so = str(tmp_path_factory.mktemp("dwfh") / "libdwfh.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, os.path.join(ROOT, "tests", "force_sensors_host.cpp")])
    lib = C.CDLL(so)
    lib.dwfh_refresh.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.POINTER(FS.DwfModel), C.POINTER(FS.DwfSensor), C.c_int] + [C.c_void_p] * 4
    lib.dwfh_pack_table.argtypes = [C.POINTER(B.DwbModel), C.c_void_p, C.c_char_p, C.c_int]
    table, err = np.zeros(B.TABLE_WORDS, np.uint32), C.create_string_buffer(256)
    m = B.model_struct(load_model())
    assert lib.dwfh_pack_table(C.byref(m), _p(table), err, 256) == 0, err.value
    lib.table = table
    return lib


def host_refresh(lib, root, dof, warm, sensors=R.DEFAULT_SENSORS, inv_dt=None, want=("sensors", "cop", "zmp", "corners"), es=None):
    n, ns = len(root), len(sensors)
    es = R.env_state_of(warm, fill=np.random.default_rng(1)) if es is None else es
    m = FS.model_struct(load_model(), R.DT)
    if inv_dt is not None:
        m.inv_dt = float(inv_dt)
    out = {"sensors": np.full((n, ns, 6), np.nan, F) if ns and "sensors" in want else None, "cop": np.full((n, 2, 4), np.nan, F) if "cop" in want else None,
           "zmp": np.full((n, 4), np.nan, F) if "zmp" in want else None, "corners": np.full((n, 8, 6), np.nan, F) if "corners" in want else None}
    rc = lib.dwfh_refresh(n, _p(lib.table), _p(np.ascontiguousarray(root, F)), _p(np.ascontiguousarray(dof, F)), _p(es), C.byref(m), c_sensors(sensors) if ns else None,
                          ns if out["sensors"] is not None else 0, _p(out["sensors"]), _p(out["cop"]), _p(out["zmp"]), _p(out["corners"]))
    assert rc == 0
    return out


def as_ref_layout(got, root):
    """The host build's (or the kernel's) rows in the pieces of R.compute, world positions turned into offsets from the base."""
    base = np.asarray(root, F).astype(np.float64)
    g = {k: v.astype(np.float64) for k, v in got.items() if v is not None}
    return {"F": g["sensors"][..., 0:3], "T": g["sensors"][..., 3:6], "cop": g["cop"], "zmp_off": g["zmp"][:, 0:2] - base[:, 0:2] * (g["zmp"][:, 2:3] > 0),
            "zmp_fz": g["zmp"][:, 2], "zmp_cnt": g["zmp"][:, 3], "cor_off": g["corners"][..., 0:3] - base[:, None, 0:3], "cor_f": g["corners"][..., 3:6]}


@pytest.fixture(scope="module", params=["float64 restatement", "g++ build"])
def impl(request, host):
    """What the known answers are asked of: (root, dof, warm, sensors) -> the pieces of R.compute."""
    if request.param == "g++ build":
        return lambda root, dof, warm, sensors=R.DEFAULT_SENSORS: as_ref_layout(host_refresh(host, root, dof, warm, sensors), root)
    return lambda root, dof, warm, sensors=R.DEFAULT_SENSORS: R.compute(root, dof, warm, R.INV_DT, sensors, np.float64)


def tol(ch):
    return R.FACTOR * R.measured()[ch]


def test_equal_normal_impulses_put_the_cop_at_the_centroid(impl):
    root, dof, _ = R.states(N, 101)
    warm = np.zeros((N, 8, 3), F)
    warm[:, :, 2] = np.random.default_rng(2).uniform(0.2, 2.0, (N, 2)).astype(F).repeat(4, 1)          # one value per sole
    _, Rf = R.foot_poses(root, dof)
    cen = R.FOOT_POS.reshape(2, 4, 3).mean(1)
    # a world-frame sensor on the world vertical through the centroid, 7 cm up: pos = centroid + R_f^T (0, 0, 0.07), per env
    for e in range(0, N, 11):
        sens = [{"foot": f, "pos": (cen[f] + Rf[e, f].T @ np.array([0, 0, 0.07])).tolist(), "world_frame": True} for f in range(2)]
        o = impl(root[e:e + 1], dof[e:e + 1], warm[e:e + 1], sens)
        assert np.abs(o["cop"][0, :, 0:2] - cen[:, 0:2]).max() <= tol("cop") and np.array_equal(o["cop"][0, :, 3], [4, 4])
        assert np.abs(o["T"][0, :, 0:2]).max() <= tol("torque") and np.abs(o["F"][0, :, 0:2]).max() == 0
        assert np.abs(o["F"][0, :, 2] - 4 * warm[e, [0, 4], 2].astype(np.float64) * float(R.INV_DT)).max() <= tol("force")


def test_one_loaded_corner_is_the_cop(impl):
    root, dof, _ = R.states(8, 102)
    for k in range(8):
        warm = np.zeros((8, 8, 3), F)
        warm[:, k] = F([0.1, -0.2, 0.9])
        o = impl(root, dof, warm)
        f = k // 4
        assert np.abs(o["cop"][:, f, 0:2] - R.FOOT_POS[k, 0:2]).max() <= tol("cop") and (o["cop"][:, f, 3] == 1).all() and not o["cop"][:, 1 - f].any()
        assert (o["zmp_cnt"] == 1).all() and np.abs(o["zmp_off"] - o["cor_off"][:, k, 0:2]).max() <= tol("zmp_off")


def test_moving_the_sensor_origin_and_changing_its_frame(impl):
    root, dof, warm = R.states(N, 103)
    a = np.array([0.03, -0.05, 0.11])
    q = np.array([0.3, -0.2, 0.5, 0.7])
    q = (q / np.linalg.norm(q)).tolist()
    p0 = np.array([0.01, 0.02, -0.09])
    sens = [{"foot": 1, "pos": p0.tolist(), "world_frame": True}, {"foot": 1, "pos": (p0 + a).tolist(), "world_frame": True},
            {"foot": 1, "pos": p0.tolist(), "quat": q, "world_frame": False}]
    o = impl(root, dof, warm, sens)
    _, Rf = R.foot_poses(root, dof)
    Ra = Rf[:, 1] @ a
    assert np.abs((o["T"][:, 1] - o["T"][:, 0]) - (-np.cross(Ra, o["F"][:, 0]))).max() <= 2 * tol("torque")
    assert np.array_equal(o["F"][:, 1], o["F"][:, 0])
    M = BR.qmat(np.asarray(q)[None])[0].T[None] @ np.swapaxes(Rf[:, 1], -1, -2)          # R(quat_s)^T R_f^T
    assert np.abs(o["F"][:, 2] - (M @ o["F"][:, 0][..., None])[..., 0]).max() <= 2 * tol("force")
    assert np.abs(o["T"][:, 2] - (M @ o["T"][:, 0][..., None])[..., 0]).max() <= 2 * tol("torque")


def test_the_cop_lies_inside_the_sole_and_zero_impulses_give_zero_rows(impl):
    root, dof, warm = R.states(512, 104)
    o = impl(root, dof, warm)
    c = R.FOOT_POS.reshape(2, 4, 3)
    lo, hi = c.min(1)[:, 0:2] - tol("cop"), c.max(1)[:, 0:2] + tol("cop")
    on = o["cop"][..., 2] > 0
    assert on.any() and (~on).any()
    assert ((o["cop"][..., 0:2] >= lo) & (o["cop"][..., 0:2] <= hi))[on].all() and not o["cop"][~on].any()
    z = impl(root, dof, np.zeros_like(warm), R.sensors8())
    for k in ("F", "T", "cop", "zmp_off", "zmp_fz", "zmp_cnt", "cor_f"):
        assert not z[k].any(), k


def test_a_nan_stays_in_its_env(host):
    root, dof, warm = R.states(5, 105)
    warm[warm == 0] = F(1e-3)          # (every corner loaded, so that the clean rows are not zero)
    clean = host_refresh(host, root, dof, warm, R.sensors8())
    warm[2, 5, 2], warm[3, 1, 0] = np.nan, np.nan
    got = host_refresh(host, root, dof, warm, R.sensors8())
    for k in clean:
        assert np.array_equal(got[k][[0, 1, 4]].view(np.uint32), clean[k][[0, 1, 4]].view(np.uint32)), k
    assert np.isnan(got["sensors"][2]).any() and np.isnan(got["sensors"][3]).any() and np.isnan(got["corners"][2, 5, 5])
    ref = R.compute(root, dof, warm, R.INV_DT, R.sensors8())
    assert np.isnan(ref["F"][2]).any() and not np.isnan(ref["F"][[0, 1, 4]]).any()


@pytest.mark.parametrize("n, sensors, xy", [(N, "default", 1.0), (N, "eight", 1.0), (5, "one", 1.0), (N, "eight", 640.0)])
def test_host_build_against_float64(host, n, sensors, xy):
    S = {"default": R.DEFAULT_SENSORS, "eight": R.sensors8(), "one": R.sensors8()[4:5]}[sensors]
    root, dof, warm = R.states(n, 111, xy=xy)
    got = host_refresh(host, root, dof, warm, S)
    ex = R.excess(got, root, dof, warm, R.INV_DT, S, report="host N=%d %s xy=%g" % (n, sensors, xy))
    assert R.within(ex) and len(ex) == 10, ex
    if xy > 100:
        assert np.abs(got["corners"][..., 0:2]).max() > 600 and np.abs(got["zmp"][:, 0:2]).max() > 600
    # every selection gives the same bits
    for want in (("cop",), ("zmp",), ("corners",), ("sensors",)):
        part = host_refresh(host, root, dof, warm, S, want=want)
        assert [k for k, v in part.items() if v is not None] == list(want)
        assert np.array_equal(part[want[0]].view(np.uint32), got[want[0]].view(np.uint32))


def test_the_base_is_added_last(host):
    """The float32 sum that adds the base FIRST misses the position allowance 640 m out; the form of the header meets it."""
    root, dof, warm = R.states(N, 112, xy=640.0)
    want = root.astype(np.float64)[:, None, 0:3] + R.compute(root, dof, warm)["cor_off"]
    c = BR.chain(root, dof, np.float32, base_first=True)          # (its "off" is the absolute position, the base added first)
    naive = np.stack([c["off"][:, R.FOOT_MV[k // 4]] + BR.mv3(c["R"][:, R.FOOT_MV[k // 4]], R.FOOT_POS[k].astype(F)[None, :]) for k in range(8)], 1)
    miss = np.abs(naive.astype(np.float64) - want) / (R.FACTOR * R.measured()["cor_off"] + R.ulp(want))
    print("base first, float32: %.1f x the allowance" % miss.max())
    assert miss.max() > 1.0


# ---------------------------------------------------------------------------------------------- 4. the CPU oracle
def test_world_frame_forces_are_the_oracles_foot_rows():
    """The CPU oracle (float build) stepped from reset with zero actions on the plane, self-collision and pushes off: nothing but the soles
    touches, so each foot's row of contact_forces is the sole solve's force alone and must equal the reference's world-frame F_w.  The robot is
    dropped from 0.93 m and lands in the fifth step.  The tolerance is force_sensors_ref.step_force_tolerance: 4 ulp of sum_k |f_k|, from the
    float32 format (measured use: printed; 0.36 of it in the landing step)."""
    from isaacgymdyros_amd.task_constants import load_task_constants
    from oracle.oracle import OracleSim
    n, steps = 3, 8
    sim = OracleSim(n, task_const=load_task_constants(), self_collision=0, perturb=0)
    sim.reset_idx(np.arange(n))
    inv_dt = F(1.0) / F(sim.cfg.dt)
    assert inv_dt == R.INV_DT
    lf, rf = sim.model.left_foot_idx, sim.model.right_foot_idx
    sens = [{"foot": 0, "world_frame": True}, {"foot": 1, "world_frame": True}]
    used, loaded_steps = 0.0, 0
    for i in range(steps):
        sim.step(np.zeros((n, 13), F), step_index=i)
        assert not sim.buf["reset_buf"].any()
        warm = abi.es_view(sim.buf["env_state"], "warm_impulses")
        cf = sim.buf["contact_forces"].astype(np.float64)
        others = [g for g in range(38) if g not in (lf, rf)]
        assert not cf[:, others].any()          # nothing but the soles touches: the feet's rows are the sole solve's alone
        ref = R.compute(sim.buf["root_states"], sim.buf["dof_state"], warm, inv_dt, sens)
        err = np.abs(ref["F"] - cf[:, [lf, rf]])
        allow = R.step_force_tolerance(warm, inv_dt)
        assert (err <= allow).all(), (i, err.max(), allow.min())
        if ref["zmp_fz"].all():
            used, loaded_steps = max(used, float((err / allow)[allow > 0].max())), loaded_steps + 1
    print("oracle: %d loaded steps, %.2f of the allowance used; total Fz %s N, weight %.1f N" % (loaded_steps, used, ref["zmp_fz"], sim.model.nominal_total_mass * 9.81))
    assert loaded_steps >= 3 and (ref["cop"][..., 2].max(1) > 0).all()          # every env has a loaded sole: not vacuous
    w = sim.buf["total_mass"].astype(np.float64) * 9.81
    assert ((ref["zmp_fz"] > w / 2) & (ref["zmp_fz"] < 2 * w)).all(), (ref["zmp_fz"], w)


# ---------------------------------------------------------------------------------------------- 5. the Python surface
def test_cfg_spec():
    assert FS.resolve(None) is None and FS.resolve(False) is None
    d = FS.resolve(True)
    assert d == FS.resolve({}) and d["cop"] is True and d["corners"] is False and d["auto"] is False
    assert [(s["body"], s["gym"], s["foot"], s["pos"], s["quat"], s["world_frame"]) for s in d["sensors"]] == \
        [("L_Foot_Link", 8, 0, [0.0, 0.0, -0.09], [0.0, 0.0, 0.0, 1.0], False), ("R_Foot_Link", 16, 1, [0.0, 0.0, -0.09], [0.0, 0.0, 0.0, 1.0], False)]
    s = FS.resolve({"sensors": [{"body": 15, "pos": [0.1, 0, 0], "quat": [0, 0, 0.6, 0.8], "world_frame": True}, {"body": "L_Foot_Redundant_Link"}, {"body": 7}],
                    "cop": False, "corners": True, "auto": True})
    assert [x["foot"] for x in s["sensors"]] == [1, 0, 0] and s["sensors"][0]["world_frame"] and abs(s["sensors"][0]["quat"][3] - 0.8) < 1e-12
    assert FS.resolve({"sensors": []})["sensors"] == []
    assert FS.foot_bodies(load_model()) == {7: 0, 8: 0, 15: 1, 16: 1}
    one = {"body": "L_Foot_Link"}
    for bad in (1, "on", [one], {"sensor": [one]}, {"sensors": one}, {"sensors": "L_Foot_Link"}, {"sensors": [one] * 9}, {"sensors": [{"body": "Head_Link"}]},
                {"sensors": [{"body": 6}]}, {"sensors": [{"body": 38}]}, {"sensors": [{"body": True}]}, {"sensors": [{"pos": [0, 0, 0]}]},
                {"sensors": [{"body": 8, "frame": "world"}]}, {"sensors": [{"body": 8, "quat": [0, 0, 0, 1.1]}]}, {"sensors": [{"body": 8, "quat": [0, 0, 0, 0]}]},
                {"sensors": [{"body": 8, "quat": [0, 0, 1]}]}, {"sensors": [{"body": 8, "pos": [0, 0]}]}, {"sensors": [{"body": 8, "pos": [0, 0, float("nan")]}]},
                {"sensors": [{"body": 8, "world_frame": 1}]}, {"cop": 1}, {"corners": "yes"}, {"auto": None}, {"zmp": True}, {"sensors": [], "cop": False}):
        with pytest.raises(ValueError):
            FS.resolve(bad)
    for mesh in ("heightfield", "trimesh"):
        with pytest.raises(ValueError, match="plane only"):
            FS.resolve(True, terrain={"mesh_type": mesh})
    assert FS.resolve(True, terrain={"mesh_type": "plane"}) == d
    from isaacgymdyros_amd.config import default_cfg, validate_cfg, with_terrain
    cfg = default_cfg(64, "cpu")
    assert "force_sensors" not in cfg["sim"]["mi355"] and "amp_force_sensors" not in cfg["sim"]["mi355"]          # (off by default)
    for key in ("force_sensors", "amp_force_sensors"):
        cfg = default_cfg(64, "cpu")
        cfg["sim"]["mi355"][key] = {"sensors": [one], "corners": True}
        validate_cfg(cfg)
        cfg["sim"]["mi355"][key] = {"sensors": [{"body": "Pelvis_Link"}]}
        with pytest.raises(ValueError):
            validate_cfg(cfg)
        cfg["sim"]["mi355"][key] = True
        with pytest.raises(ValueError, match="plane only"):
            validate_cfg(with_terrain(cfg, mesh_type="heightfield"))
