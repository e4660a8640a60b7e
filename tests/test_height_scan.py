"""The terrain height scan without a GPU (include/dyros_height_scan.h, isaacgymdyros_amd/csrc/dw_height_scan.h): the
header, the Python binding and the built library agree; the numpy restatement of the header (tests/height_scan_ref.py) against the
REFERENCE's recorded get_heights (tests/golden/height_scan_ref.npz) at every point that is not near a sample line, and the mistakes that
check must reject; the per-env arithmetic -- compiled by g++ from the header the HIP kernel includes (tests/height_scan_host.cpp) -- bit for
bit against the restatement, on, just below and just above sample lines too; the bilinear rule and the probes within 4 d of float64 on the
scenes of tests/terrain_edge_cases.py; the exact properties; refusals; the Python layer; the kernel's resources.

The fixture check has two parts.  The issue's: equality with the reference at every point that is not near a line.  And, asking more: equality
at the near-line points too.  The fixture stands two envs on sample lines with yaw exactly 0 (282 of 26 880 points near a line, 1.05 %), where
the reference's cell is decided by its own addition and division alone, and the restatement with gpu_div = 0 equals the reference at all of
them: the header's order is the reference's own to the bit.  That second part is what rejects the multiply form under gpu_div = 0 (88 of the
282 differ): the two forms differ by at most 1.5 ulp of the coordinate, inside the band of 4 d_u, so no point that is not near a line can
tell them apart (0 of 26 598 differ).  The other six mistakes are rejected by the first part alone."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import height_scan_ref as R
import inverse_dynamics_resources as RES
import terrain_edge_cases as TE
from isaacgymdyros_amd import body_states as BS
from isaacgymdyros_amd import build, cbind, config
from isaacgymdyros_amd import height_scan as H
from isaacgymdyros_amd import model_tensors as MT
from isaacgymdyros_amd.model import load_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dw_height_scan.hip"
F = np.float32
K = H.K
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "height_scan_ref.npz"))
FIELDS = ("field_rough", "field_stairs", "field_tiny")
OBS = (float(GOLD["obs_offset"]), float(GOLD["obs_clip"]), float(GOLD["obs_scale"]))
SCENES = ("borders", "borders_no_border", "lines", "scales_h0.07", "scales_h0.25", "scales_h0.5", "scales_h1.0")
OUTPUTS = ("heights", "points", "obs", "probe_pos", "probe_height", "clearance", "probe_normal")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------------------------------------- 1. the ABI
@pytest.fixture(scope="module")
def api():
    return H.declare(C.CDLL(build.build()))


def test_header_python_and_library_agree(api):
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dyros_height_scan.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(dwh_[a-z_0-9]+)\s*\(", src)))
    assert declared == sorted("dwh_" + n for n in H.EXPORTS) == ["dwh_abi_version", "dwh_last_error", "dwh_pack_table", "dwh_scan"]
    assert dict(build.SOURCES)[SRC] == ["-ffp-contract=off"] and "dw_height_scan.h" in build.HEADERS
    syms = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout.split()
    assert sorted(s for s in syms if s.startswith("dwh_")) == declared
    assert api["abi_version"]() == K["DWH_ABI_VERSION"] == 1
    assert api["scan"].argtypes == [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] * 2 + [C.c_float] * 3 + [C.c_int32] * 2 + [C.c_void_p] * 8
    assert K["DWH_T_NP"] == BS.K["DWB_TABLE_WORDS"] and K["DWH_T_WALK"] + 2 * K["DWH_MAX_PROBES"] == K["DWH_T_PROBE"]
    assert K["DWH_T_PROBE"] + K["DWH_PROBE_WORDS"] * K["DWH_MAX_PROBES"] == K["DWH_T_GRID"]
    assert K["DWH_T_GRID"] + 2 * K["DWH_MAX_POINTS"] == K["DWH_TABLE_WORDS"] and K["DWH_TABLE_WORDS"] % 4 == 0
    assert K["DWH_MAX_POINTS"] >= 4 * 140 and K["DWH_MAX_PROBES"] >= 16 and C.sizeof(H.DwhProbe) == 16 and C.sizeof(H.DwhParams) == 32
    assert H.DEFAULTS == {"grid": None, "rule": "nearest", "probes": "soles", "normals": False, "points": False, "obs": None, "auto": False}


def test_scan_refusals_happen_before_any_launch(api):
    """Every buffer is NULL or a host address here: a launch would fault, a refusal returns -1 with its message."""
    one = C.c_void_p(16)
    ok = dict(n=8, table=one, root=one, dof=one, hs=one, rows=4, cols=4, hscale=0.1, vscale=0.005, border=0.0, rule=0, div=0, heights=one)

    def call(**kw):
        a = dict(ok, **kw)
        outs = [a.get(k) for k in OUTPUTS]
        return api["scan"](a["n"], a["table"], a["root"], a["dof"], a["hs"], a["rows"], a["cols"], a["hscale"], a["vscale"], a["border"], a["rule"],
                           a["div"], *outs, None)
    for kw, msg in ((dict(n=0), b"num_envs"), (dict(table=None), b"a buffer is missing"), (dict(root=None), b"a buffer is missing"),
                    (dict(dof=None), b"a buffer is missing"), (dict(heights=None), b"at least one output"),
                    (dict(table=C.c_void_p(4)), b"16-byte aligned"), (dict(rule=2), b"rule must be"), (dict(rows=1), b"2 x 2"),
                    (dict(cols=1), b"2 x 2"), (dict(rows=8193), b"8192"), (dict(hscale=0.0), b"hscale and vscale"),
                    (dict(hscale=float("nan")), b"hscale and vscale"), (dict(vscale=-1.0), b"hscale and vscale"),
                    (dict(vscale=float("inf")), b"hscale and vscale"), (dict(border=float("nan")), b"border must be finite")):
        assert call(**kw) == -1 and msg in api["last_error"](), (kw, api["last_error"]())


def test_pack_table_refusals(api):
    model, grid = load_model(), H.default_grid()
    soles = H.resolve(True)["probes"]
    t = H.pack_table(api, model, grid, soles, H.params_struct(70, 90, 0.1, 0.005, 2.0))
    assert t.dtype == np.uint32 and t.shape == (K["DWH_TABLE_WORDS"],)
    assert np.array_equal(t[:BS.K["DWB_TABLE_WORDS"]], BS.pack_table(BS.declare(C.CDLL(build.build())), model))
    assert t[K["DWH_T_NP"]] == 140 and t[K["DWH_T_NB"]] == 8 and t[K["DWH_T_NW"]] == 2          # the eight corners share two walks: the two legs
    assert t[K["DWH_T_WALK"]:K["DWH_T_WALK"] + 4].tolist() == [0, 6, 1, 6]
    assert np.array_equal(t[K["DWH_T_GRID"]:K["DWH_T_GRID"] + 280].view(F).reshape(140, 2), grid)
    # the base gets a walk of depth 0; a body up the arm one of its own
    t2 = H.pack_table(api, model, grid[:1], [{"gym": 0, "pos": [0, 0, 0]}, {"gym": 37, "pos": [0, 0, 0.1]}], H.params_struct())
    assert t2[K["DWH_T_NW"]] == 2 and t2[K["DWH_T_WALK"] + 1] == 0 and t2[K["DWH_T_WALK"] + 3] > 0

    def refused(msg, model=model, grid=grid, probes=soles, **prm):
        p = dict(rows=70, cols=90, hscale=0.1, vscale=0.005, border=2.0)
        p.update(prm)
        obs = {k[4:]: p.pop(k) for k in list(p) if k.startswith("obs_")}
        with pytest.raises(cbind.DyrosWalkLibraryError, match=msg):
            H.pack_table(api, model, grid, probes, H.params_struct(obs=obs, **p))
    import copy
    bad = copy.deepcopy({k: model.d[k] for k in ("mv_parent", "mv_pos", "mv_rot0", "mv_axis", "body_moving", "inert_gym", "inert_mv", "inert_mass", "inert_com")})
    bad["mv_parent"][5] = 6
    refused("dwh_pack_table: a child precedes its parent", model=bad)          # what dwb_pack_table refuses, under this entry point's name
    refused("grid points must be in 1..DWH_MAX_POINTS", grid=np.zeros((K["DWH_MAX_POINTS"] + 1, 2), F))
    refused("probes must be in 0..DWH_MAX_PROBES", probes=[{"gym": 0, "pos": [0, 0, 0]}] * (K["DWH_MAX_PROBES"] + 1))
    refused("a grid offset is not finite", grid=np.array([[0, 0], [np.inf, 0]], F))
    refused("a grid offset is not finite", grid=np.array([[0, np.nan]], F))
    refused("a probe's point is not finite", probes=[{"gym": 3, "pos": [0, np.nan, 0]}])
    refused("unknown body", probes=[{"gym": 38, "pos": [0, 0, 0]}])
    refused("unknown body", probes=[{"gym": -1, "pos": [0, 0, 0]}])
    for k in ("hscale", "vscale"):
        for v in (0.0, -0.1, float("nan"), float("inf")):
            refused(k + " must be finite and > 0", **{k: v})
    refused("border must be finite", border=float("nan"))
    refused("at least 2 x 2", rows=1)
    refused("at least 2 x 2", cols=0)
    refused("8192", rows=8193)
    refused("obs parameters", obs_clip=-1.0)
    refused("obs parameters", obs_scale=float("nan"))
    with pytest.raises(cbind.DyrosWalkLibraryError, match="grid points must be in"):
        cbind.check(api, api["pack_table"](C.byref(BS.model_struct(model)), grid.ctypes.data, 0, None, 0, C.byref(H.params_struct()), t.ctypes.data))


# ---------------------------------------------------------------------------------------------- 2. the kernel's resources
def test_one_kernel_without_scratch():
    ks = RES.kernels(SRC)
    assert len(ks) == 1 and "dwh_k_scan" in next(iter(ks))
    r = next(iter(ks.values()))
    print("dwh_k_scan: %d VGPRs, scratch %d B, LDS %d B, occupancy %d" % (r["vgprs"], r["scratch"], r["lds"], r["occ"]))
    assert r["scratch"] == 0 and r["lds"] <= 64 * 1024 and r["vgprs"] <= 128


# ---------------------------------------------------------------------------------------------- 3. the restatement against the reference
def gold_case(c):
    hs = GOLD[FIELDS[int(GOLD["case_field"][c])]]
    return hs, float(GOLD["case_hscale"][c]), float(GOLD["vscale"]), float(GOLD["case_border"][c])


def fixture_check(bug=None, gpu_div=0):
    """(held points that differ, near-line points that differ, held points) of the restatement against the fixture, heights and obs."""
    wrong = near_wrong = held = 0
    for c in range(len(GOLD["root"])):
        hs, hscale, vscale, border = gold_case(c)
        got = R.grid32(GOLD["root"][c], GOLD["grid"], hs, hscale, vscale, border, "nearest", gpu_div, OBS, bug)
        diff = (bits(got["heights"]) != bits(GOLD["heights"][c])) | (bits(got["obs"]) != bits(GOLD["obs"][c]))
        near = GOLD["near"][c]
        wrong, near_wrong, held = wrong + int((diff & ~near).sum()), near_wrong + int((diff & near).sum()), held + int((~near).sum())
    return wrong, near_wrong, held


def test_fixture_meets_its_condition():
    near, du = GOLD["near"], float(GOLD["d_u"])
    assert near.mean() <= R.NEAR_CAP and 0 < du < 1e-4
    assert near[0, 0].all() and near[2, 0].all() and near.sum() >= 280          # the two envs that stand on sample lines
    again = 0.0
    for c in range(len(GOLD["root"])):          # d_u and the band are what this helper computes from the same inputs
        _, hscale, _, border = gold_case(c)
        again = max(again, R.d_u_of(GOLD["root"][c], GOLD["grid"], border, hscale))
        assert np.array_equal(R.near_line(*R.coords64(GOLD["root"][c], GOLD["grid"], border, hscale), du), near[c])
    assert again == du
    # the fixture reaches what it is meant to: all four sides outside the map, tilts up to 1 rad, the whole circle of yaw
    r = GOLD["root"].reshape(-1, 13).astype(np.float64)
    tilt = 2 * np.arcsin(np.clip(np.hypot(r[:, 3], r[:, 4]), 0, 1))
    yaw = 2 * np.arctan2(r[:, 5], r[:, 6])
    assert tilt.max() > 0.9 and np.histogram(np.mod(yaw, 2 * np.pi), bins=8, range=(0, 2 * np.pi))[0].min() > 0
    assert len(np.unique(GOLD["heights"])) > 20 and np.abs(GOLD["obs"]).max() == 5.0 and (np.abs(GOLD["obs"]) < 5.0).any()


def test_default_grid_is_the_references():
    assert np.array_equal(bits(H.default_grid()), bits(GOLD["grid"])) and H.default_grid().shape == (140, 2)
    assert np.array_equal(bits(H.resolve(True)["grid"]), bits(GOLD["grid"]))


def test_restatement_equals_the_reference_away_from_lines():
    wrong, near_wrong, held = fixture_check()
    print("restatement against the reference: %d of %d held points differ; %d of %d near-line points differ" % (wrong, held, near_wrong, int(GOLD["near"].sum())))
    assert wrong == 0 and held >= 0.98 * GOLD["near"].size
    assert near_wrong == 0          # (asks more than the issue: on the lines the placed envs stand on, the reference rounds as the header does)


@pytest.mark.parametrize("bug", R.BUGS)
def test_the_fixture_check_rejects(bug):
    wrong, near_wrong, held = fixture_check(bug)
    print("%s: %d of %d held points differ; %d near-line points differ" % (bug, wrong, held, near_wrong))
    if bug == "multiply_under_cpu_div":          # no point away from a line can tell the two forms apart (the module's docstring): the placed envs do
        assert wrong == 0 and near_wrong > 0
    else:
        assert wrong > 0


# ---------------------------------------------------------------------------------------------- 4. the g++ build
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/height_scan_host.cpp")
    so = str(tmp_path_factory.mktemp("dwhh") / "libdwhh.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "emul"),
                           '-DDW_HOST_SHIM_HEADER="dw_wave_host.h"', '-DDWQ_HOST_SHIM_HEADER="dw_quad_wave_host.h"', "-o", so,
                           os.path.join(ROOT, "tests", "height_scan_host.cpp")])
    lib = C.CDLL(so)
    lib.dwhh_scan.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_float] * 3 + [C.c_int] * 2 + [C.c_void_p] * 7
    lib.dwhh_pack_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    return lib


MODEL_C = BS.model_struct(load_model())
SOLES = H.resolve(True)["probes"]


def host_table(host, grid, probes=(), obs=None, prm=()):
    g, t, err = np.ascontiguousarray(grid, F).reshape(-1, 2), np.zeros(K["DWH_TABLE_WORDS"], np.uint32), C.create_string_buffer(256)
    arr, p = H.probe_array(list(probes)), H.params_struct(*prm, obs=obs)
    rc = host.dwhh_pack_table(C.byref(MODEL_C), _p(g), len(g), arr, len(probes), C.byref(p), _p(t), err, 256)
    assert rc == 0, err.value
    return t


def host_scan(host, table, root, dof, hs, hscale=0.1, vscale=0.005, border=0.0, rule=0, gpu_div=0, want=OUTPUTS, fill=None):
    """dict of the requested outputs from the g++ build; fill: the value the buffers hold before (to see what is written)."""
    n, P, B = len(root), int(table[K["DWH_T_NP"]]), int(table[K["DWH_T_NB"]])
    root = np.ascontiguousarray(root, F)
    dof = np.zeros((n, 33, 2), F) if dof is None else np.ascontiguousarray(dof, F)
    shapes = dict(heights=(n, P), points=(n, P, 2), obs=(n, P), probe_pos=(n, B, 3), probe_height=(n, B), clearance=(n, B), probe_normal=(n, B, 3))
    out = {k: np.full(shapes[k], np.nan if fill is None else fill, F) for k in want}
    hs = None if hs is None else np.ascontiguousarray(hs, np.int16)
    rows, cols = (0, 0) if hs is None else hs.shape
    assert host.dwhh_scan(n, _p(table), _p(root), _p(dof), _p(hs), rows, cols, hscale, vscale, border, rule, gpu_div, *[_p(out.get(k)) for k in OUTPUTS]) == 0
    return out


@pytest.mark.parametrize("gpu_div", (0, 1))
@pytest.mark.parametrize("rule", ("nearest", "bilinear"))
def test_host_build_equals_the_restatement_bit_for_bit(host, rule, gpu_div):
    t = host_table(host, GOLD["grid"], obs=dict(zip(("offset", "clip", "scale"), OBS)))
    for c in range(len(GOLD["root"])):
        hs, hscale, vscale, border = gold_case(c)
        want = R.grid32(GOLD["root"][c], GOLD["grid"], hs, hscale, vscale, border, rule, gpu_div, OBS)
        got = host_scan(host, t, GOLD["root"][c], None, hs, hscale, vscale, border, H.RULES[rule], gpu_div, ("heights", "points", "obs"))
        for k in ("heights", "points", "obs"):
            assert np.array_equal(bits(got[k]), bits(want[k])), (c, k)
    if rule == "nearest" and gpu_div == 0:          # and so the g++ build equals the reference
        for c in range(len(GOLD["root"])):          # (near the lines too, the placed envs of cases 0 and 2 among them)
            got = host_scan(host, t, GOLD["root"][c], None, *gold_case(c), 0, 0, ("heights",))["heights"]
            assert np.array_equal(bits(got), bits(GOLD["heights"][c])), c


def line_cases(field):
    """Roots with yaw 0 whose grid point of offset (0, 0) lies just below, on and just above sample lines (terrain_edge_cases.line_floats),
    per axis, the other coordinate mid-cell; beside the zero offset the grid holds offsets of whole and half samples."""
    rows = []
    for ax, n in enumerate((field.tot_rows, field.tot_cols)):
        for k in (1, 7, 23, 35, n - 3, n - 2, n - 1):          # (not line 20, world 0: the floats there are far denser than the coordinate's)
            for x in TE.line_floats(field, k, ax):
                if x is not None:
                    r = np.zeros(13, F)
                    r[ax], r[1 - ax], r[6], r[2] = x, F(1.234), 1.0, 0.9
                    rows.append(r)
    grid = np.array([[0, 0], [0.1, 0], [0, 0.1], [-0.2, 0.3], [0.05, -0.05], [0.5, 0.5]], F)
    return np.stack(rows), grid


@pytest.mark.parametrize("gpu_div", (0, 1))
def test_host_build_on_sample_lines(host, gpu_div):
    field = TE.scene("lines")[0]
    root, grid = line_cases(field)
    args = (field.heightsamples, field.hscale, field.vscale, field.border)
    t = host_table(host, grid, obs={})
    for rule in ("nearest", "bilinear"):
        want = R.grid32(root, grid, *args, rule, gpu_div, (0.5, 1.0, 1.0))
        got = host_scan(host, t, root, None, *args, H.RULES[rule], gpu_div, ("heights", "points", "obs"))
        for k in ("heights", "points", "obs"):
            assert np.array_equal(bits(got[k]), bits(want[k])), (rule, k)
    # the placement bites: on these points the two forms of the coordinate give different cells
    a = R.grid32(root, grid, *args, "nearest", 0)["heights"]
    b = R.grid32(root, grid, *args, "nearest", 1)["heights"]
    print("points on which gpu_div decides the cell: %d of %d" % (int((a != b).sum()), a.size))
    assert (a != b).any()


@pytest.mark.parametrize("name", SCENES)
def test_bilinear_and_probes_within_4d_of_float64(host, name):
    field, root, dof, _ = TE.scene(name)
    grid = GOLD["grid"]
    args = (field.heightsamples, field.hscale, field.vscale, field.border)
    t = host_table(host, grid, SOLES)
    d = R.channel_d(field, t, grid, SOLES, name)
    got = host_scan(host, t, root, dof, *args, H.RULES["bilinear"], 1)
    check_against_float64(field, root, dof, grid, SOLES, got, d, name)


def check_against_float64(field, root, dof, grid, probes, got, d, label):
    """Holds the bilinear heights and the probe channels of `got` within 4 d of float64; the normals only away from lines (cap 2 %)."""
    b = R.truth64(field, root, dof, grid, probes)
    for k, ref in (("heights", "bilinear"), ("points", "points"), ("probe_pos", "probe_pos"), ("probe_height", "probe_height"), ("clearance", "clearance")):
        if k in got:
            err = float(np.abs(got[k] - b[ref]).max())
            print("%-18s %-13s err %.3e  d %.3e" % (label, k, err, d[ref]))
            assert err <= 4 * d[ref], (label, k, err, d[ref])
    if "probe_normal" in got:
        near = R.probe_near(field, b["probe_pos"], got["probe_pos"])
        if near.mean() > R.NEAR_CAP:          # (the `lines` scene PUTS corners on lines, more than the cap allows to leave out; it is one plane, so every probe is held)
            near[:] = False
        err = float(np.abs(got["probe_normal"] - b["probe_normal"])[~near].max())
        print("%-18s %-13s err %.3e  d %.3e  (%d of %d probes near a line)" % (label, "probe_normal", err, d["probe_normal"], int(near.sum()), near.size))
        assert err <= 4 * d["probe_normal"], (label, err, d["probe_normal"], near.mean())


# ---------------------------------------------------------------------------------------------- 5. the exact properties
def test_exact_properties(host):
    hs, hscale, vscale, border = gold_case(0)
    root, grid = GOLD["root"][0].copy(), GOLD["grid"]
    t = host_table(host, grid, SOLES)
    base = host_scan(host, t, root, None, hs, hscale, vscale, border, 0, 0)
    # the root's z, the pitch and the roll never enter the grid: another z, and x and y of the quaternion scaled (another tilt, the same z and w)
    other = root.copy()
    other[:, 2] += 0.37
    other[:, 3:5] *= F(0.25)
    got = host_scan(host, t, other, None, hs, hscale, vscale, border, 0, 0, ("heights", "points"))
    assert np.array_equal(bits(got["heights"]), bits(base["heights"])) and np.array_equal(bits(got["points"]), bits(base["points"]))
    # P changes no point's bits: a prefix, one point, and the cap
    for P in (1, 63, 64, 65, K["DWH_MAX_POINTS"]):
        g = np.concatenate([grid] * 8)[:P]
        part = host_scan(host, host_table(host, g), root, None, hs, hscale, vscale, border, 0, 0, ("heights",))["heights"]
        assert np.array_equal(bits(part), bits(np.concatenate([base["heights"]] * 8, 1)[:, :P])), P
    # outputs that are not requested are not written; B = 0 leaves the probe outputs alone
    for k in OUTPUTS:
        one = host_scan(host, t, root, None, hs, hscale, vscale, border, 0, 0, (k,), fill=7.0)
        assert (one[k] != 7.0).any() and np.array_equal(bits(one[k]), bits(base[k])), k
    none = host_scan(host, host_table(host, grid), root, None, hs, hscale, vscale, border, 0, 0, OUTPUTS, fill=7.0)
    assert all((none[k] == 7.0).all() for k in OUTPUTS[3:]) and np.array_equal(bits(none["heights"]), bits(base["heights"]))
    # the plane: +0.0, (0, 0, 1), clearance = z
    pl = host_scan(host, t, root, None, None)
    assert not bits(pl["heights"]).any() and not bits(pl["probe_height"]).any() and np.array_equal(bits(pl["clearance"]), bits(pl["probe_pos"][..., 2]))
    assert (pl["probe_normal"] == np.array([0, 0, 1], F)).all() and np.array_equal(bits(pl["points"]), bits(base["points"]))
    # a non-finite env: NaN in its outputs, its neighbours keep their bits
    bad = root.copy()
    bad[3, 9], bad[5, 0] = np.inf, np.nan
    dof = np.zeros((len(root), 33, 2), F)
    dof[7, 11, 0] = np.nan
    dof[8, 11, 1] = np.nan          # (a joint RATE is not looked at)
    ref = host_scan(host, t, root, np.zeros_like(dof), hs, hscale, vscale, border, 0, 0)
    got = host_scan(host, t, bad, dof, hs, hscale, vscale, border, 0, 0)
    for k in OUTPUTS:
        assert np.isnan(got[k][[3, 5, 7]]).all() and np.array_equal(bits(np.delete(got[k], [3, 5, 7], 0)), bits(np.delete(ref[k], [3, 5, 7], 0))), k


def test_an_env_640_m_out_reads_the_same_heights(host):
    """On a field with a period of 8 samples at hscale 0.25 (2 m), the same state moved 640 m = 2560 samples along x gets the same bits of
    `heights` at every point farther than 1e-3 grid units from a line (one ulp of 640 m is 6.1e-5 m = 2.4e-4 grid units)."""
    rng = np.random.default_rng(5)
    tile = rng.integers(-8, 9, size=(8, 8)).astype(np.int16)
    hs = np.tile(tile, (330, 2))          # 2640 x 16
    root = GOLD["root"][0].copy()
    root[:, 0], root[:, 1] = rng.uniform(2.0, 6.0, len(root)).astype(F), rng.uniform(1.2, 2.4, len(root)).astype(F)
    far = root.copy()
    far[:, 0] += F(640.0)
    grid = H.mesh(0.1 * np.arange(-3, 4), 0.1 * np.arange(-3, 4))
    t = host_table(host, grid)
    a = host_scan(host, t, root, None, hs, 0.25, 0.005, 0.0, 0, 1, ("heights",))["heights"]
    b = host_scan(host, t, far, None, hs, 0.25, 0.005, 0.0, 0, 1, ("heights",))["heights"]
    u, v = R.coords64(root, grid, 0.0, 0.25)
    away = ~R.near_line(u, v, 1e-3 / 4)
    assert away.mean() > 0.95 and np.array_equal(bits(a)[away], bits(b)[away]) and len(np.unique(a)) > 8


# ---------------------------------------------------------------------------------------------- 6. the Python layer
def test_resolve_and_validate():
    assert H.resolve(None) is None and H.resolve(False) is None
    s = H.resolve({})
    assert s["rule_id"] == 0 and [p["gym"] for p in s["probes"]] == [f["gym"] for f in load_model().foot_pts] and s["obs"] is None
    assert H.resolve({"probes": None})["probes"] == [] and H.resolve({"obs": {}})["obs"] == {"offset": 0.5, "clip": 1.0, "scale": 1.0}
    g = H.resolve({"grid": {"x": [0.0, 0.5], "y": [-0.1, 0.0, 0.1]}})["grid"]
    assert g.tolist() == np.array([[0, -0.1], [0, 0], [0, 0.1], [0.5, -0.1], [0.5, 0], [0.5, 0.1]], F).tolist()          # x-major
    assert H.resolve({"grid": [[0.25, -1.0]], "rule": "bilinear"})["rule_id"] == 1
    p = H.resolve({"probes": [{"body": "Head_Link"}, {"body": 0, "pos": [0.1, 0, 0]}]})["probes"]
    assert p[0]["pos"] == [0.0, 0.0, 0.0] and p[1]["body"] == load_model().body_names[0]
    for bad, msg in ((3, "must be True, False or a dict"), ({"grids": 1}, "unknown keys"), ({"auto": 1}, "auto must be"), ({"normals": "x"}, "normals must be"),
                     ({"rule": "linear"}, "rule must be"), ({"grid": []}, "1..1024 points"), ({"grid": [[0, 0]] * 1025}, "1..1024 points"),
                     ({"grid": {"x": [0]}}, "x and y"), ({"grid": [[0, float("nan")]]}, "finite"), ({"grid": "all"}, "grid must be"),
                     ({"probes": "feet"}, "probes must be"), ({"probes": [{"body": "Nose"}]}, "neither a body name"), ({"probes": [{"body": 38}]}, "neither a body name"),
                     ({"probes": [{"pos": [0, 0, 0]}]}, "a probe is a dict"), ({"probes": [{"body": 0, "pos": [0, 0]}]}, "3 finite numbers"),
                     ({"probes": [{"body": 0}] * 17}, "at most 16"), ({"probes": None, "normals": True}, "no probe"),
                     ({"obs": 3}, "obs must be"), ({"obs": {"gain": 1}}, "obs must be"), ({"obs": {"clip": -1}}, "clip must be"), ({"obs": {"scale": "x"}}, "finite numbers")):
        with pytest.raises(ValueError, match=msg):
            H.validate(bad)
    with pytest.raises(ValueError, match="horizontal_scale must be finite and > 0"):
        H.validate(True, {"mesh_type": "trimesh", "horizontal_scale": 0.0})
    H.validate(True, {"mesh_type": "trimesh"})
    H.validate(True, {"mesh_type": "plane"})          # accepted on the plane
    # through validate_cfg, under either task's key
    for key in ("height_scan", "amp_height_scan"):
        cfg = config.default_cfg(4)
        cfg["sim"]["mi355"][key] = {"rule": "cubic"}
        with pytest.raises(ValueError, match="rule must be"):
            config.validate_cfg(cfg)
        cfg["sim"]["mi355"][key] = {"obs": {}, "rule": "bilinear"}
        config.validate_cfg(config.with_terrain(cfg, mesh_type="trimesh"))


def test_sensors_are_walked_after_solvers_and_off_by_default(monkeypatch):
    assert MT.SENSORS == (("height_scan", "HeightScan", ("terrain",)),)
    assert [r[0] for r in MT._all()] == [r[0] for r in MT.FEATURES] + [r[0] for r in MT.SOLVERS] + ["height_scan"]
    env = types.SimpleNamespace()
    MT.attach(env, env, {})          # the key absent: None, nothing loaded or allocated
    assert env.height_scan is None and all(getattr(env, r[0]) is None for r in MT._all())
    MT.attach(env, env, {"height_scan": False, "amp_height_scan": True})
    assert env.height_scan is None
    order = []
    for name, _, _ in MT._all():
        setattr(env, name, types.SimpleNamespace(auto=True, refresh=lambda name=name: order.append(name)))
    MT.refresh_auto(env)
    assert order == [r[0] for r in MT._all()] and order[-1] == "height_scan"
    seen = []
    monkeypatch.setattr(H, "validate", lambda spec, terrain=None: seen.append((spec, terrain)))
    MT.validate_all({"sim": {"mi355": {"height_scan": True}}, "terrain": {"mesh_type": "trimesh"}})
    assert seen == [(True, {"mesh_type": "trimesh"})]
    # the product does not reach into the tests or the oracle
    src = open(os.path.join(ROOT, "isaacgymdyros_amd", "height_scan.py")).read()
    assert "oracle" not in src and "tests" not in re.sub(r'""".*?"""', "", src, flags=re.S)
