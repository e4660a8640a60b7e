"""The rigid-body state tensor without a GPU (include/dyros_bodies.h, isaacgymdyros_amd/csrc/dw_bodies.h): the header, the
Python binding and the built library agree; refusals; the kernel's resources; the per-env arithmetic -- compiled by g++ from the header the HIP
kernel includes (tests/body_states_host.cpp) -- against the float64 restatement of tests/body_states_ref.py under its measured tolerance; the
rows' structure; the reference's own velocities against central differences of its own poses; the welded foot bodies in the MJCF."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import body_states_ref as R
from isaacgymdyros_amd import body_states as B
from isaacgymdyros_amd import build, cbind
from isaacgymdyros_amd.model import MODEL_JSON, compile_mjcf, load_model
from test_gait_profile_abi import TAKEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dw_bodies.hip"
N = 67
SUBSET = [37, 0, 16, 8, 8]
MJCF = os.path.join(os.environ.get("DW_REFERENCE", "/root/reference"), "python/IsaacGymEnvs/assets/mjcf/dyros_tocabi/xml/dyros_tocabi.xml")          # (as tools/compile_assets.py)
F = np.float32


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------- 1. the ABI
def declared():
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dyros_bodies.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dwb_[a-z_0-9]+)\s*\(", src)))


@pytest.fixture(scope="module")
def api():
    return cbind.declare(C.CDLL(build.build()), "dyros_bodies.h", "dwb_")


def test_header_python_and_library_agree(api):
    assert declared() == sorted("dwb_" + n for n in B.EXPORTS) == ["dwb_abi_version", "dwb_last_error", "dwb_pack_table", "dwb_refresh"]
    assert dict(build.SOURCES)[SRC] == ["-ffp-contract=off"] and "dw_bodies.h" in build.HEADERS
    lib = C.CDLL(build.build())
    for fn in declared():
        assert hasattr(lib, fn), fn
    assert lib.dwb_abi_version() == B.K["DWB_ABI_VERSION"] == 1
    assert api["refresh"].argtypes == [C.c_int32] + [C.c_void_p] * 5 + [C.c_int32] * 2 + [C.c_void_p] * 3 and api["refresh"].restype is C.c_int
    assert api["pack_table"].argtypes == [C.POINTER(B.DwbModel), C.c_void_p] and api["last_error"].restype is C.c_char_p
    K = B.K
    assert (K["DWB_NUM_BODIES"], K["DWB_NUM_MOVING"], K["DWB_NUM_DOF"], K["DWB_NUM_INERT"], K["DWB_ROW"]) == (38, 34, 33, 36, 13)
    # the table's sections follow one another and fit
    assert K["DWB_T_PATHLEN"] == K["DWB_T_NLEAF"] + 1 and K["DWB_T_PATH"] == K["DWB_T_PATHLEN"] + K["DWB_MAX_LEAVES"]
    assert K["DWB_T_MV"] == K["DWB_T_PATH"] + K["DWB_MAX_LEAVES"] * K["DWB_MAX_DEPTH"]
    assert K["DWB_T_CARRIER"] == K["DWB_T_MV"] + 34 * K["DWB_MV_WORDS"] and K["DWB_T_RECORD"] == K["DWB_T_CARRIER"] + 38
    assert K["DWB_T_INERT"] == K["DWB_T_RECORD"] + 38 and K["DWB_T_INERT"] + 36 * K["DWB_INERT_WORDS"] <= K["DWB_TABLE_WORDS"]
    assert K["DWB_TABLE_WORDS"] % 4 == 0 and C.sizeof(B.DwbModel) == 4 * (34 * 16 + 38 + 36 * 6)


def test_refusals_happen_before_any_launch(api):
    """Every buffer is NULL or a host address here: a launch would fault, a refusal returns -1 with its message."""
    one = C.c_void_p(16)
    ids = (C.c_int32 * 2)(0, 38)
    for args, msg in (((0, one, one, one, None, None, 0, 0, one, one, None), b"num_envs"),
                      ((8, None, one, one, None, None, 0, 0, one, one, None), b"a buffer is missing"),
                      ((8, one, None, one, None, None, 0, 0, one, one, None), b"a buffer is missing"),
                      ((8, one, one, None, None, None, 0, 0, one, one, None), b"a buffer is missing"),
                      ((8, one, one, one, None, None, 0, 0, None, None, None), b"states or com"),
                      ((8, one, one, one, None, None, 5, 0, one, one, None), b"nb must be 0 or 38"),
                      ((8, one, one, one, None, ids, 0, 0, one, one, None), b"nb must be in 1..38"),
                      ((8, one, one, one, None, ids, 39, 0, one, one, None), b"nb must be in 1..38"),
                      ((8, one, one, one, None, ids, 2, 0, one, one, None), b"outside 0..37"),
                      ((8, C.c_void_p(4), one, one, None, None, 0, 0, one, one, None), b"16-byte aligned")):
        assert api["refresh"](*args) == -1 and msg in api["last_error"](), (args, api["last_error"]())


def test_pack_table_validates_the_model(api):
    d = load_model().d
    t = B.pack_table(api, d)
    K = B.K
    assert t.dtype == np.uint32 and t.shape == (K["DWB_TABLE_WORDS"],)
    # TOCABI: five leaves -- the two ankles, the two wrists, the head -- at depths 6, 6, 11, 5, 11
    assert t[K["DWB_T_NLEAF"]] == 5 and t[K["DWB_T_PATHLEN"]:K["DWB_T_PATHLEN"] + 8].tolist() == [6, 6, 11, 5, 11, 0, 0, 0]
    paths = t[K["DWB_T_PATH"]:K["DWB_T_MV"]].reshape(8, 12)
    assert (paths[0, :6] & 255).tolist() == [1, 2, 3, 4, 5, 6] and (paths[3, :5] & 255).tolist() == [13, 14, 15, 24, 25]
    owned = sorted(int(x & 255) for x in paths.ravel() if x & K["DWB_PATH_OWNER"])
    assert owned == list(range(1, 34))          # every moving body below the base is stored by exactly one path
    assert t[K["DWB_T_CARRIER"]:K["DWB_T_CARRIER"] + 38].tolist() == d["body_moving"]
    rec = t[K["DWB_T_RECORD"]:K["DWB_T_RECORD"] + 38].view(np.int32).tolist()
    assert rec == R.RECORD and rec[7] == rec[15] == -1
    q0 = t[K["DWB_T_MV"]:K["DWB_T_CARRIER"]].view(F).reshape(34, 11)[:, 4:8]
    assert np.abs(q0.astype(np.float64) - R.MV_Q0).max() < 2e-7 and (q0[:, 3] > -1e-6).all()

    def refused(msg, **change):
        import copy
        bad = copy.deepcopy({k: d[k] for k in ("mv_parent", "mv_pos", "mv_rot0", "mv_axis", "body_moving", "inert_gym", "inert_mv", "inert_mass", "inert_com")})
        for k, (i, v) in change.items():
            bad[k][i] = v
        with pytest.raises(cbind.DyrosWalkLibraryError, match=msg):
            B.pack_table(api, bad)
    refused("a child precedes its parent", mv_parent=(5, 6))
    refused("mv_parent out of range", mv_parent=(5, 34))
    refused("body_moving out of range", body_moving=(7, 34))
    refused("body_moving out of range", body_moving=(7, -1))
    refused("inert_gym out of range", inert_gym=(3, 38))
    refused("inert_mv out of range", inert_mv=(3, -2))
    refused("two inertial records", inert_gym=(7, 6))          # (record 7 is Gym body 8's, on the same carrier as Gym body 6)
    refused("not its Gym body's carrier", inert_mv=(3, 4))


# ---------------------------------------------------------------------------------------------- 2. the kernel's resources
@pytest.fixture(scope="module")
def remarks():
    extra = dict(build.SOURCES)[SRC]
    cmd = [build.hipcc()] + build.FLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(build.CSRC, SRC)]
    return subprocess.run(cmd, cwd=build.CSRC, capture_output=True, text=True, check=True).stderr


def test_kernels_use_no_scratch_and_fit_the_lds(remarks):
    names = re.findall(r"remark: Function Name: (\S+)", remarks)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)]
    assert len(names) >= 1 and len(scratch) == len(lds) == len(names)
    for n, s, l in zip(names, scratch, lds):
        assert "dwb_k_" in n and s == 0 and l <= 65536, (n, s, l)
        assert not any(x in n for x in TAKEN + ("dwg_k_",)), n


# ---------------------------------------------------------------------------------------------- 3. the g++ build against float64
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/body_states_host.cpp")
    so = str(tmp_path_factory.mktemp("dwbh") / "libdwbh.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, os.path.join(ROOT, "tests", "body_states_host.cpp")])
    lib = C.CDLL(so)
    lib.dwbh_refresh.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 2 + [C.c_void_p] * 2
    lib.dwbh_pack_table.argtypes = [C.POINTER(B.DwbModel), C.c_void_p, C.c_char_p, C.c_int]
    table, err = np.zeros(B.TABLE_WORDS, np.uint32), C.create_string_buffer(256)
    m = B.model_struct(load_model())
    assert lib.dwbh_pack_table(C.byref(m), _p(table), err, 256) == 0, err.value
    lib.table = table
    return lib


def host_refresh(lib, root, dof, ms, vel_at_com, ids=None, states=True, com=True):
    n, nb = len(root), 38 if ids is None else len(ids)
    st = np.full((n, nb, 13), np.nan, F) if states else None
    cm = np.full((n, 7), np.nan, F) if com else None
    arr = None if ids is None else np.asarray(ids, np.int32)
    assert lib.dwbh_refresh(n, _p(lib.table), _p(root), _p(dof), _p(ms), _p(arr), nb, vel_at_com, _p(st), _p(cm)) == 0
    return st, cm


def test_the_library_and_the_host_build_pack_the_same_table(api, host):
    assert np.array_equal(B.pack_table(api, load_model()), host.table)


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_host_build_against_float64(host, vel_at_com):
    root, dof, ms = R.states(N, 11 + vel_at_com, mass=True)
    st, cm = host_refresh(host, root, dof, ms, vel_at_com)
    ex = R.excess(st, cm, root, dof, ms, vel_at_com, report="host N=%d vel_at_com=%d" % (N, vel_at_com))
    assert R.within(ex), ex
    # a subset with a repeat: the full tensor's rows bit for bit; states only, com only, no mass scale
    sub, none = host_refresh(host, root, dof, ms, vel_at_com, ids=SUBSET, com=False)
    assert none is None and np.array_equal(sub.view(np.uint32), st[:, SUBSET].view(np.uint32))
    assert R.within(R.excess(sub, None, root, dof, ms, vel_at_com, ids=SUBSET))
    _, cm1 = host_refresh(host, root, dof, None, vel_at_com, states=False)
    assert R.within(R.excess(None, cm1, root, dof, None, vel_at_com))
    total = float(np.sum(load_model().inert_mass))
    assert np.abs(cm1[:, 6].astype(np.float64) - total).max() <= R.FACTOR * R.measured(vel_at_com)["mass"]


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_rows_structure(host, vel_at_com):
    root, dof, ms = R.states(N, 21, mass=True)
    st, _ = host_refresh(host, root, dof, ms, vel_at_com)
    u = st.view(np.uint32)
    assert np.array_equal(u[:, 0], root.view(np.uint32))          # row 0 is the root row, bit for bit
    for carrier, welded in ((6, (7, 8)), (14, (15, 16))):
        for g in welded:
            assert np.array_equal(u[:, g, 0:7], u[:, carrier, 0:7]) and np.array_equal(u[:, g, 10:13], u[:, carrier, 10:13])
            if not vel_at_com:
                assert np.array_equal(u[:, g, 7:10], u[:, carrier, 7:10])
    if vel_at_com:
        # Gym 6, 8, 14 and 16 have inertial records of their own, so their COM velocities differ; Gym 7 and 15 have none and give the
        # carrier origin's velocity, which the reference restates
        assert not np.array_equal(u[:, 8, 7:10], u[:, 6, 7:10]) and not np.array_equal(u[:, 7, 7:10], u[:, 6, 7:10])
        c = R.chain(root, dof, np.float64, 1)
        assert np.abs(st[:, [7, 15], 7:10] - c["vo"][:, [6, 12]]).max() <= R.FACTOR * R.measured(1)["vel"]


def test_offsets_are_as_accurate_640_m_out(host):
    """The float32 recursion that adds the base FIRST misses the position allowance 640 m out; the form of the header meets it."""
    root, dof, ms = R.states(N, 31, xy=640.0)
    st, cm = host_refresh(host, root, dof, ms, 1)
    ex = R.excess(st, cm, root, dof, ms, 1, report="host 640 m")
    assert R.within(ex), ex
    naive = R.chain(root, dof, np.float32, 1, base_first=True)
    want = root.astype(np.float64)[:, None, 0:3] + R.chain(root, dof, np.float64, 1)["off"]
    err = np.abs(naive["off"].astype(np.float64) - want)
    miss = err / (R.FACTOR * R.measured(1)["off"] + R.ulp(want))
    print("base first, float32: %.2e m off, %.1f x the allowance" % (err.max(), miss.max()))
    assert miss.max() > 1.0


def test_non_finite_inputs_stay_in_their_env(host):
    root, dof, ms = R.states(5, 41)
    clean, ccom = host_refresh(host, root, dof, ms, 1)
    root[2, 4], dof[3, 20, 0] = np.nan, np.inf
    st, cm = host_refresh(host, root, dof, ms, 1)
    keep = [0, 1, 4]
    assert np.array_equal(st[keep].view(np.uint32), clean[keep].view(np.uint32)) and np.array_equal(cm[keep].view(np.uint32), ccom[keep].view(np.uint32))
    assert not np.isfinite(st[2, 1:, 3:7]).any() and not np.isfinite(st[3, 27, 3:7]).all() and not np.isfinite(cm[[2, 3], 0:3]).any()


# ---------------------------------------------------------------------------------------------- 4. the reference itself
def test_reference_chain_agrees_with_fk():
    """Positions and rotations of the quaternion chain against tests/terrain_edge_cases.py fk (matrices, the same float64 model constants): two
    ways to write one chain, equal to rounding."""
    from terrain_edge_cases import fk
    root, dof, _ = R.states(256, 51)
    c = R.chain(root, dof)
    x, Rm = fk(root.astype(np.float64), dof[..., 0].astype(np.float64))
    assert np.abs(c["root"][:, None, 0:3] + c["off"] - x).max() < 1e-12 and np.abs(c["R"] - Rm).max() < 1e-12


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_reference_velocities_are_the_derivatives_of_its_poses(vel_at_com):
    """Central differences, h = 1e-6, of the reference's own positions and rotations, the state advanced by its own velocities, at 4096
    states.  The bound, 1e-6 m/s and 1e-6 rad/s, is a fifth of the float32 recursion's d for these channels (5e-6, 6e-6), so the reference's
    own error cannot eat the margin of four.  What to expect: truncation h^2 |d3x/dt3| / 6 < 1e-8 and rounding 2^-52 |x| / h about 2e-10 per
    term of an 11-deep sum."""
    h = 1e-6
    root, dof, _ = R.states(4096, 61)
    root, dof = root.astype(np.float64), dof.astype(np.float64)
    c = R.chain(root, dof, np.float64, vel_at_com)

    def advanced(s):
        r2, d2 = root.copy(), dof.copy()
        r2[:, 0:3] += s * h * c["vo"][:, 0]
        w = root[:, 10:13]
        a = np.linalg.norm(w, axis=1, keepdims=True) * s * h
        dq = np.concatenate([w / np.linalg.norm(w, axis=1, keepdims=True) * np.sin(a / 2), np.cos(a / 2)], 1)
        r2[:, 3:7] = R.qmul(dq, root[:, 3:7])
        d2[..., 0] += s * h * dof[..., 1]
        return R.chain(r2, d2)
    cp, cm = advanced(+1.0), advanced(-1.0)
    xp, xm = cp["root"][:, None, 0:3] + cp["off"], cm["root"][:, None, 0:3] + cm["off"]
    ev = np.abs((xp - xm) / (2 * h) - c["vo"]).max()
    W = ((cp["R"] - cm["R"]) / (2 * h)) @ np.swapaxes(c["R"], -1, -2)          # [w]x
    ew = np.abs(np.stack([W[..., 2, 1], W[..., 0, 2], W[..., 1, 0]], -1) - c["w"]).max()
    ec = 0.0
    if vel_at_com:          # the rows' velocities are those of the bodies' COMs, x_m + R_m c_g; the base's is the root row's own
        r1 = R.rows(c, 1)
        assert np.abs(r1["vel"][:, 0] - root[:, 7:10]).max() < 1e-12
        for g in range(R.NB):
            if R.RECORD[g] >= 0:
                m, cg = R.CARRIER[g], R.INERT_COM[R.RECORD[g]].astype(np.float64)
                pp, pm = xp[:, m] + R.mv3(cp["R"][:, m], cg), xm[:, m] + R.mv3(cm["R"][:, m], cg)
                ec = max(ec, float(np.abs((pp - pm) / (2 * h) - r1["vel"][:, g]).max()))
    print("finite differences: origin velocity %.2e m/s, angular velocity %.2e rad/s, COM velocity %.2e m/s" % (ev, ew, ec))
    assert ev < 1e-6 and ew < 1e-6 and ec < 1e-6


# ---------------------------------------------------------------------------------------------- 5. the Python surface
def test_cfg_spec_and_selection():
    names = load_model().body_names
    assert B.resolve(None) is None and B.resolve(False) is None
    assert B.resolve(True) == B.resolve({}) == {"bodies": None, "com": True, "auto": False, "ids": list(range(38))}
    s = B.resolve({"bodies": ["Head_Link", 8, "R_Foot_Link", 8], "com": False, "auto": True})
    assert s["ids"] == [29, 8, 16, 8] and s["com"] is False and s["auto"] is True
    for bad in (1, "on", [8], {"body": [8]}, {"bodies": []}, {"bodies": [38]}, {"bodies": [-1]}, {"bodies": ["Tail_Link"]}, {"bodies": "Head_Link"},
                {"bodies": [True]}, {"bodies": list(range(38)) + [0]}, {"com": 1}, {"auto": "yes"}):
        with pytest.raises(ValueError):
            B.resolve(bad)
    assert B.select_parents(list(range(38)), load_model().body_parent) == load_model().body_parent
    # head, left foot, its carrier's parent, pelvis: only the pelvis is anybody's parent here, and of nobody selected directly
    assert B.select_parents([29, 8, 5, 0, 6, 8], load_model().body_parent) == [-1, 4, -1, -1, 2, 4]
    assert names[29] == "Head_Link" and names[8] == "L_Foot_Link" and names[16] == "R_Foot_Link"
    from isaacgymdyros_amd.config import default_cfg, validate_cfg
    cfg = default_cfg(64, "cpu")
    assert "body_states" not in cfg["sim"]["mi355"]          # (off by default)
    cfg["sim"]["mi355"]["body_states"] = {"bodies": ["Head_Link", "L_Foot_Link", "R_Foot_Link"]}
    validate_cfg(cfg)
    cfg["sim"]["mi355"]["body_states"] = {"bodies": ["Head"]}
    with pytest.raises(ValueError):
        validate_cfg(cfg)


# ---------------------------------------------------------------------------------------------- 6. the MJCF (reference-live)
@pytest.mark.skipif(not os.path.exists(MJCF), reason="the reference checkout is not present")
def test_welded_foot_bodies_sit_on_their_carriers_in_the_mjcf():
    import json
    import xml.etree.ElementTree as ET
    bodies = {b.get("name"): b for b in ET.parse(MJCF).getroot().iter("body")}
    for name in ("L_Foot_Redundant_Link", "L_Foot_Link", "R_Foot_Redundant_Link", "R_Foot_Link"):
        b = bodies[name]
        assert b.find("joint") is None and b.get("quat") is None and [float(x) for x in b.get("pos", "0 0 0").split()] == [0.0, 0.0, 0.0], name
    with open(MODEL_JSON) as f:
        assert compile_mjcf(MJCF) == json.load(f)
