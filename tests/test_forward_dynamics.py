"""The forward dynamics without a GPU (include/dyros_forward_dynamics.h, isaacgymdyros_amd/csrc/dw_factor.h): the
reference (tests/forward_dynamics_ref.py) against things that are not itself -- L' D L against M, the dense forward dynamics, the inverse
dynamics; the per-env arithmetic -- compiled by g++ from the headers the HIP kernel includes (tests/forward_dynamics_host.cpp) -- against the
float64 reference under its measured tolerance and under the derived backward-error bound; the outputs' exact properties; the header, the
Python binding and the built library; refusals; the kernel's resources; the cfg surface."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import body_states_ref as R
import dynamics_ref as DR
import forward_dynamics_ref as FR
import jacobians_ref as JR
from isaacgymdyros_amd import build, cbind
from isaacgymdyros_amd import forward_dynamics as FM
from isaacgymdyros_amd import jacobians as JM
from isaacgymdyros_amd.model import load_model
from test_body_states import TAKEN as TAKEN_BODIES          # noqa: F401
from test_gait_profile_abi import TAKEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dw_forward_dynamics.hip"
N = 37
F = np.float32
U = np.uint32
OUTS = ("x", "factor", "minv")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------- 1. the reference against what is not itself
def test_the_pattern_is_the_trees():
    """396 words, 17 in a row at the most, and exactly where two coordinates can couple: jacobians_ref.branch_mask's lower triangle."""
    assert FR.PATTERN == 396 and max(len(c) for c in FR.ROWS) == 17
    assert np.array_equal(FR.MASK, np.tril(JR.branch_mask()))
    assert all(c == sorted(c) and c[-1] == r for r, c in enumerate(FR.ROWS))


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_reference_factor_reconstructs_the_mass_matrix(vel_at_com):
    """L' D L == M in float64 at 64 seeded states: 17 products per entry of up to |M| <= 100, so 64 ulp of the largest entry is ample; and the
    pattern loses nothing: the sweeps agree with np.linalg.solve to the conditioning (4e4) times round-off."""
    root, dof, ms, arm, _acc = DR.seeded(64, 3 + vel_at_com)
    M = FR.mass_matrix(root, dof, vel_at_com, ms, arm)
    L, D = FR.ltdl(M)
    err = np.abs(np.einsum("nki,nk,nkj->nij", L, D, L) - M).max()
    assert (D > 0).all() and err <= 64 * 2.0 ** -52 * np.abs(M).max(), err
    assert (L[:, ~(FR.MASK | np.eye(39, dtype=bool))] == 0).all()
    rhs = FR.rhs_of(root, dof, vel_at_com, ms, arm, 2, 5).astype(np.float64)
    want = np.swapaxes(np.linalg.solve(M, np.swapaxes(rhs, 1, 2)), 1, 2)
    got = FR.solve(L, D, rhs)
    print("L' D L against M: %.2e; the sweeps against np.linalg.solve: %.2e on values up to %.0f" % (err, np.abs(got - want).max(), np.abs(want).max()))
    assert np.abs(got - want).max() <= 1e5 * 2.0 ** -52 * np.abs(want).max()


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_reference_against_the_dense_forward_dynamics(vel_at_com):
    """DenseDynamics.accelerations with zero damping, dt = 0 and seeded joint torques, converted to our coordinates as tests/test_dynamics.py
    does, against M^-1 ([0; tau] - h) with h of dynamics_ref.  Both solve a system of condition number up to 4e4 in float64: 1e-8 of the
    largest acceleration is a thousand times their round-off and a hundred thousandth of the float32 d."""
    from dense_dynamics_np import DenseDynamics, body_twist_from_root
    model = load_model()
    dd = DenseDynamics(model)
    n = 8
    root, dof, ms, arm, _acc = DR.seeded(n, 5)
    r64, d64, ms64, arm64 = root.astype(np.float64), dof.astype(np.float64), ms.astype(np.float64), arm.astype(np.float64)
    G64 = np.asarray(DR.GRAVITY, F).astype(np.float64)
    tau = np.random.default_rng(91).normal(0, 50, (n, 33))
    c = R.chain(root, dof, np.float64, vel_at_com)
    pr = JR.p_ref(c, vel_at_com)
    acc = np.zeros((n, 39))
    for e in range(n):
        nu_b = body_twist_from_root(r64[e], model.inert_com[R.RECORD[0]], bool(vel_at_com))
        ab, qdd, t = dd.accelerations(r64[e, 0:3], r64[e, 3:7], d64[e, :, 0], nu_b, d64[e, :, 1], ms64[e], arm64[e], np.zeros(33), 0.0, G64, tau[e])
        R0 = t["Rw"][0]
        om, al = R0 @ nu_b[0:3], R0 @ ab[0:3]
        xdd = R0 @ ab[3:6] + np.cross(om, R0 @ nu_b[3:6])
        acc[e, 0:3] = xdd + np.cross(al, pr[e]) + np.cross(om, np.cross(om, pr[e]))
        acc[e, 3:6], acc[e, 6:] = al, qdd
    h = DR.evaluate(root, dof, vel_at_com, ms, arm, c=c)["bias"]
    M = JR.mass_matrix(c, vel_at_com, ms, arm)[0]
    L, D = FR.ltdl(M)
    rhs = np.concatenate([np.zeros((n, 6)), tau], 1) - h
    got = FR.solve(L, D, rhs[:, None])[:, 0]
    err = np.abs(got - acc).max()
    print("M^-1 ([0; tau] - h) against the dense forward dynamics: %.2e with |a| up to %.0f" % (err, np.abs(acc).max()))
    assert err <= 1e-8 * np.abs(acc).max()


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_reference_forward_of_inverse_is_the_identity(vel_at_com):
    """forward(inverse(a)) == a with dynamics_ref.evaluate's tau = M a + h (36 dense Jacobians, no mass matrix), to the same 1e-8."""
    root, dof, ms, arm, acc = DR.seeded(16, 7)
    out = DR.evaluate(root, dof, vel_at_com, ms, arm, acc.astype(np.float64))
    M = FR.mass_matrix(root, dof, vel_at_com, ms, arm)
    L, D = FR.ltdl(M)
    got = FR.solve(L, D, (out["tau"] - out["bias"])[:, None])[:, 0]
    err = np.abs(got - acc.astype(np.float64)).max()
    print("forward(inverse(a)) - a: %.2e with |a| up to %.0f" % (err, np.abs(acc).max()))
    assert err <= 1e-8 * np.abs(acc).max()


# ---------------------------------------------------------------------------------------------- 2. the g++ build against float64
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/forward_dynamics_host.cpp")
    so = str(tmp_path_factory.mktemp("dwlh") / "libdwlh.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, os.path.join(ROOT, "tests", "forward_dynamics_host.cpp")])
    so_j = str(tmp_path_factory.mktemp("dwlh") / "libdwjh.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", so_j, os.path.join(ROOT, "tests", "jacobians_host.cpp")])
    lib = C.CDLL(so)
    lib.dwlh_solve.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    lib.dwlh_pack_table.argtypes = [C.POINTER(JM.DwjModel), C.c_void_p, C.c_char_p, C.c_int]
    table, err = np.zeros(FM.TABLE_WORDS, U), C.create_string_buffer(256)
    m = JM.model_struct(load_model())
    assert lib.dwlh_pack_table(C.byref(m), _p(table), err, 256) == 0, err.value
    lib.table = table
    lib.jac = C.CDLL(so_j)
    lib.jac.dwjh_mass_matrix.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 2
    return lib


def host_run(lib, root, dof, ms, arm, vel_at_com, rhs=None, sub=None, outs=OUTS, pattern=False, expect=0):
    """The outputs named, NaN-filled beforehand, as a dict (the others None; "pattern_m" when asked)."""
    n = len(root)
    nrhs = 0 if rhs is None else rhs.shape[1]
    o = {"x": np.full((n, nrhs, 39), np.nan, F) if "x" in outs and rhs is not None else None,
         "factor": np.full((n, 39, 39), np.nan, F) if "factor" in outs else None, "minv": np.full((n, 39, 39), np.nan, F) if "minv" in outs else None}
    pm = np.full((n, FM.PATTERN), np.nan, F) if pattern else None
    rc = lib.dwlh_solve(n, _p(lib.table), _p(root), _p(dof), _p(ms), _p(arm), vel_at_com, _p(rhs), nrhs, _p(sub), _p(o["x"]), _p(o["factor"]), _p(o["minv"]), _p(pm))
    assert rc == expect
    if pattern:
        o["pattern_m"] = pm
    return o


def host_mass_matrix(lib, root, dof, ms, arm, vel_at_com):
    mm = np.full((len(root), 39, 39), np.nan, F)
    assert lib.jac.dwjh_mass_matrix(len(root), _p(lib.table), _p(root), _p(dof), _p(ms), _p(arm), vel_at_com, _p(mm), None) == 0
    return mm


def test_the_library_and_the_host_build_pack_the_same_table(host):
    api = cbind.declare(C.CDLL(build.build()), "dyros_forward_dynamics.h", "dwl_")
    japi = cbind.declare(C.CDLL(build.build()), "dyros_jacobians.h", "dwj_")
    t = FM.pack_table(api, load_model())
    K = FM.K
    assert t.dtype == U and t.shape == (FM.TABLE_WORDS,) and np.array_equal(t, host.table)
    assert np.array_equal(t[:K["DWL_T_ROW"]], JM.pack_table(japi, load_model()))
    # the new sections are the pattern the reference derives from mv_parent
    assert np.array_equal(t[K["DWL_T_ROW"]:K["DWL_T_COL"]].astype(np.int64), FR.ROW_START)
    assert np.array_equal(t[K["DWL_T_COL"]:K["DWL_T_TROW"]].astype(np.int64), FR.COLS)
    assert np.array_equal(t[K["DWL_T_TROW"]:K["DWL_T_TCOL"]].astype(np.int64), FR.TCOL_START)
    assert np.array_equal(t[K["DWL_T_TCOL"]:-3].astype(np.int64), FR.TCOLS) and (t[-3:] == 0).all()
    # it refuses what dwj_pack_table refuses, under its own name
    d = {k: np.array(v) for k, v in load_model().d.items() if k in ("mv_parent", "mv_pos", "mv_rot0", "mv_axis", "body_moving", "inert_gym", "inert_mv", "inert_mass",
                                                                     "inert_com", "inert_I")}
    d["mv_parent"][5] = 6
    with pytest.raises(cbind.DyrosWalkLibraryError, match="dwl_pack_table: a child precedes its parent"):
        FM.pack_table(api, d)
    d["mv_parent"][5] = load_model().d["mv_parent"][5]
    d["inert_I"][9][1][1] = float("nan")
    with pytest.raises(cbind.DyrosWalkLibraryError, match="dwl_pack_table: inert_I is not finite"):
        FM.pack_table(api, d)


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_host_build_against_float64(host, vel_at_com):
    """Every channel within 4 d of the float64 reference; M's pattern words are the bits of the g++ build of dwj_mass_matrix; and L' D L formed in
    float64 from the factor agrees with that M within 2 gamma_18 (|L'| |D| |L|)_ij."""
    root, dof, ms, arm, _acc = DR.seeded(N, 11 + vel_at_com)
    rhs = FR.rhs_of(root, dof, vel_at_com, ms, arm, 2, 17)
    sub = DR.evaluate(root, dof, vel_at_com, ms, arm)["bias"].astype(F)
    o = host_run(host, root, dof, ms, arm, vel_at_com, rhs, sub, pattern=True)
    ex = FR.excess({k: o[k] for k in OUTS}, root, dof, ms, arm, vel_at_com, rhs, sub, report="host N=%d vel_at_com=%d" % (N, vel_at_com))
    assert len(ex) == len(FR.CHANNELS) and FR.within(ex), ex
    mm = host_mass_matrix(host, root, dof, ms, arm, vel_at_com)
    assert np.array_equal(o["pattern_m"].view(U), mm[:, FR.COLS >> 8, FR.COLS & 255].view(U))
    assert (mm[:, ~(FR.MASK | FR.MASK.T)] == 0).all()
    be = FR.backward_error(o["factor"], mm)
    print("host: L' D L against M: %.3f of 2 gamma_18 |L'| |D| |L|" % be)
    assert be <= 1.0
    # nominal masses, no armature: another matrix, under the d measured for it (one mode: the measurement takes its time)
    if vel_at_com == 0:
        return
    rhs = FR.rhs_of(root, dof, vel_at_com, None, None, 1, 19)
    o = host_run(host, root, dof, None, None, vel_at_com, rhs)
    ex = FR.excess(o, root, dof, None, None, vel_at_com, rhs, report="host, nominal masses, no armature")
    assert FR.within(ex), ex
    assert FR.backward_error(o["factor"], host_mass_matrix(host, root, dof, None, None, vel_at_com)) <= 1.0


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_exact_properties(host, vel_at_com):
    root, dof, ms, arm, _acc = DR.seeded(N, 21)
    R8 = FM.MAX_RHS
    rhs = FR.rhs_of(root, dof, vel_at_com, ms, arm, R8, 23)
    o = host_run(host, root, dof, ms, arm, vel_at_com, rhs)
    assert all(np.isfinite(o[k]).all() for k in OUTS)
    # 640 m out: the same bits
    far = root.copy()
    far[:, 0:2] += np.array([640.0, -640.0], F)
    of = host_run(host, far, dof, ms, arm, vel_at_com, rhs)
    assert all(np.array_equal(of[k].view(U), o[k].view(U)) for k in OUTS)
    # the factor: +0.0 above the diagonal and at all 384 lower entries outside the pattern; D positive
    f = o["factor"]
    outside = ~FR.MASK
    assert outside.sum() == 39 * 39 - 396 and np.tril(outside).sum() == 384 + 0 and (f.view(U)[:, outside] == 0).all()
    assert (f[:, np.arange(39), np.arange(39)] > 0).all()
    # minv: symmetric bit for bit, and column c is the solve of the identity's column c
    assert np.array_equal(o["minv"].view(U), np.swapaxes(o["minv"], 1, 2).view(U))
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(39, dtype=F)[:R8], (N, R8, 39)))
    oe = host_run(host, root, dof, ms, arm, vel_at_com, eye, outs=("x",))
    assert all(np.array_equal(oe["x"][:, c, c:].view(U), o["minv"][:, c:, c].view(U)) for c in range(R8))
    # column r is the same bits at nrhs = 1, 2 and the maximum
    for k in (1, 2):
        ok = host_run(host, root, dof, ms, arm, vel_at_com, np.ascontiguousarray(rhs[:, :k]), outs=("x",))
        assert np.array_equal(ok["x"].view(U), o["x"][:, :k].view(U)), k
    last = host_run(host, root, dof, ms, arm, vel_at_com, np.ascontiguousarray(rhs[:, R8 - 1:]), outs=("x",))
    assert np.array_equal(last["x"][:, 0].view(U), o["x"][:, R8 - 1].view(U))
    # sub NULL equals sub of zeros; a zero right-hand side gives zeros; rhs = sub gives zeros
    oz = host_run(host, root, dof, ms, arm, vel_at_com, rhs, np.zeros((N, 39), F), outs=("x",))
    assert np.array_equal(oz["x"].view(U), o["x"].view(U))
    assert (host_run(host, root, dof, ms, arm, vel_at_com, np.zeros((N, 2, 39), F), outs=("x",))["x"] == 0).all()
    same = np.ascontiguousarray(rhs[:, :1])
    assert (host_run(host, root, dof, ms, arm, vel_at_com, same, np.ascontiguousarray(same[:, 0]), outs=("x",))["x"] == 0).all()
    # with the armature off M's diagonal lacks it: D[38], the last row's own entry of M, is smaller by exactly that armature, to rounding
    on = host_run(host, root, dof, ms, None, vel_at_com, pattern=True, outs=("factor",))
    ow = host_run(host, root, dof, ms, arm, vel_at_com, pattern=True, outs=("factor",))
    diag = FR.ROW_START[1:] - 1
    assert np.array_equal((on["pattern_m"][:, diag[6:]] + arm).view(U), ow["pattern_m"][:, diag[6:]].view(U))
    assert np.array_equal(on["pattern_m"][:, diag[:6]].view(U), ow["pattern_m"][:, diag[:6]].view(U))
    assert np.array_equal(on["factor"][:, 38, 38].view(U), on["pattern_m"][:, -1].view(U)) and (on["factor"][:, 38, 38] < ow["factor"][:, 38, 38]).all()


def test_a_null_output_leaves_the_others_bits(host):
    root, dof, ms, arm, _acc = DR.seeded(N, 31)
    rhs = FR.rhs_of(root, dof, 1, ms, arm, 3, 33)
    full = host_run(host, root, dof, ms, arm, 1, rhs)
    for k in OUTS:
        one = host_run(host, root, dof, ms, arm, 1, rhs if k == "x" else None, outs=(k,))
        assert np.array_equal(one[k].view(U), full[k].view(U)) and all(one[j] is None for j in OUTS if j != k), k
        rest = host_run(host, root, dof, ms, arm, 1, None if k == "x" else rhs, outs=tuple(j for j in OUTS if j != k))
        assert all(np.array_equal(rest[j].view(U), full[j].view(U)) for j in OUTS if j != k), k


def test_non_finite_inputs_stay_in_their_env(host):
    root, dof, ms, arm, _acc = DR.seeded(6, 41)
    rhs = FR.rhs_of(root, dof, 1, ms, arm, 2, 43)
    o0 = host_run(host, root, dof, ms, arm, 1, rhs)
    root[2, 4], dof[3, 20, 0], rhs[5, 1, 7] = np.nan, np.inf, np.nan
    o = host_run(host, root, dof, ms, arm, 1, rhs)
    for k in OUTS:
        assert np.array_equal(o[k][[0, 1, 4]].view(U), o0[k][[0, 1, 4]].view(U)), k
        assert np.isnan(o[k][2]).any() and np.isnan(o[k][3]).any(), k
    # a NaN in one right-hand side reaches that column of x alone
    assert np.isnan(o["x"][5, 1]).any() and np.array_equal(o["x"][5, 0].view(U), o0["x"][5, 0].view(U))
    assert all(np.array_equal(o[k][5].view(U), o0[k][5].view(U)) for k in ("factor", "minv"))


# ---------------------------------------------------------------------------------------------- 3. the ABI
@pytest.fixture(scope="module")
def api():
    return cbind.declare(C.CDLL(build.build()), "dyros_forward_dynamics.h", "dwl_")


@pytest.mark.parametrize("check", ["prototypes", "layouts"])
def test_header_python_and_library_agree(check, tmp_path):
    import test_cbind as TC
    if check == "prototypes":
        TC.test_ctypes_prototypes_match_the_header("dyros_forward_dynamics.h", "dwl_", "forward_dynamics", C.CDLL(build.build()))
    else:
        TC.test_struct_layouts_match_the_host_compiler("dyros_forward_dynamics.h", "dwl_", "forward_dynamics", tmp_path)          # (it declares no struct of its own)
    assert sorted(FM.EXPORTS) == ["abi_version", "last_error", "pack_table", "solve"]
    assert dict(build.SOURCES)[SRC] == ["-ffp-contract=off"] and "dw_factor.h" in build.HEADERS
    K, KJ = FM.K, JM.K
    assert K["DWL_ABI_VERSION"] == 1 and (K["DWL_NV"], K["DWL_PATTERN"], K["DWL_MAX_ROW"]) == (39, 396, 17)
    for name in ("NUM_BODIES", "NUM_MOVING", "NUM_DOF", "NV"):
        assert K["DWL_" + name] == KJ["DWJ_" + name]
    assert K["DWL_T_ROW"] == KJ["DWJ_TABLE_WORDS"] and K["DWL_T_COL"] == K["DWL_T_ROW"] + 40 and K["DWL_T_TROW"] == K["DWL_T_COL"] + 396
    assert K["DWL_T_TCOL"] == K["DWL_T_TROW"] + 40 and K["DWL_TABLE_WORDS"] == K["DWL_T_TCOL"] + 357 + 3
    assert K["DWL_TABLE_WORDS"] % 4 == 0 and K["DWL_GROUP"] * K["DWL_LANES"] == 256 and 1 <= K["DWL_MAX_RHS"] <= 64
    assert FM.DEFAULTS == {"rhs": 1, "factor": False, "minv": False, "armature": True, "auto": False}
    text = open(os.path.join(ROOT, "include", "dyros_forward_dynamics.h")).read()
    assert "is NOT the inverse of mass_matrix[:, 6:, 6:]" in text and "NOT the inverse of jacobians.mm" in FM.__doc__
    # the older headers are untouched
    assert KJ["DWJ_ABI_VERSION"] == 1 and cbind.constants("dyros_dynamics.h", "dwn_")["DWN_ABI_VERSION"] == 1


def test_refusals_happen_before_any_launch(api):
    """Every buffer is NULL or a host address here: a launch would fault, a refusal returns -1 with its message."""
    one = C.c_void_p(16)
    ok = lambda **kw: tuple(dict(dict(n=8, table=one, root=one, dof=one, ms=None, arm=None, vac=0, rhs=one, nrhs=1, sub=None, x=one, factor=None,          # noqa: E731
                                      minv=None, stream=None), **kw).values())
    for args, msg in ((ok(n=0), b"num_envs"), (ok(n=-3), b"num_envs"), (ok(n=1 << 30), b"num_envs"),
                      (ok(table=None), b"a buffer is missing"), (ok(root=None), b"a buffer is missing"), (ok(dof=None), b"a buffer is missing"),
                      (ok(table=C.c_void_p(8)), b"16-byte aligned"),
                      (ok(x=None), b"rhs needs x"), (ok(x=None, factor=one), b"rhs needs x"),
                      (ok(rhs=None), b"x needs rhs"), (ok(rhs=None, minv=one), b"x needs rhs"),
                      (ok(rhs=None, x=None, sub=one, factor=one), b"sub needs rhs"),
                      (ok(nrhs=0), b"nrhs"), (ok(nrhs=-1), b"nrhs"), (ok(nrhs=FM.MAX_RHS + 1), b"nrhs"),
                      (ok(rhs=None, x=None), b"no output"), (ok(rhs=None, x=None, nrhs=0), b"no output")):
        assert api["solve"](*args) == -1 and msg in api["last_error"]() and b"dwl_solve" in api["last_error"](), (args, api["last_error"]())


# ---------------------------------------------------------------------------------------------- 4. the kernel's resources
@pytest.fixture(scope="module")
def remarks():
    extra = dict(build.SOURCES)[SRC]
    cmd = [build.hipcc()] + build.FLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(build.CSRC, SRC)]
    return subprocess.run(cmd, cwd=build.CSRC, capture_output=True, text=True, check=True).stderr


def test_kernel_uses_no_scratch_and_fits_the_lds(remarks):
    names = re.findall(r"remark: Function Name: (\S+)", remarks)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)]
    assert len(names) == 1 and len(scratch) == len(lds) == len(names)
    assert "dwl_k_solve" in names[0]
    for n, s, l in zip(names, scratch, lds):
        # five workgroups to a CU's 160 KB
        assert "dwl_k_" in n and s == 0 and l <= 32768, (n, s, l)
        assert not any(x in n for x in tuple(TAKEN) + tuple(TAKEN_BODIES) + ("dwg_k_", "dwb_k_", "dwf_k_", "dwj_k_", "dwn_k_")), n
        assert not any(x in n for x in ("k_mlp", "k_wgrad", "k_policy", "k_adam", "k_grad_stats", "k_finish", "k_gae", "k_roll_pre", "k_roll_post", "k_loss",
                                        "k_relu_bwd", "k_bias_relu", "k_stage_obs", "k_retile", "dw_k_amp", "dw_k_newwalk", "dw_k_body_positions")), n
    print("dwl_k_solve: LDS %d bytes per workgroup" % lds[0])


# ---------------------------------------------------------------------------------------------- 5. the Python surface
def test_cfg_spec():
    full = {"rhs": 1, "factor": False, "minv": False, "armature": True, "auto": False}
    assert FM.resolve(None) is None and FM.resolve(False) is None
    assert FM.resolve(True) == FM.resolve({}) == full
    s = FM.resolve({"rhs": 3, "factor": True, "minv": True, "auto": True, "armature": False})
    assert s == {"rhs": 3, "factor": True, "minv": True, "armature": False, "auto": True}
    assert FM.resolve({"rhs": FM.MAX_RHS})["rhs"] == FM.MAX_RHS
    for bad in (1, "on", ["minv"], {"h": True}, {"factor": 1}, {"minv": None}, {"armature": 1.0}, {"auto": "no"}, {"rhs": 0}, {"rhs": FM.MAX_RHS + 1}, {"rhs": True},
                {"rhs": 2.0}, {"rhs": "1"}, {1: True}):
        with pytest.raises(ValueError):
            FM.resolve(bad)
    from isaacgymdyros_amd.config import default_cfg, validate_cfg
    cfg = default_cfg(64, "cpu")
    assert "forward_dynamics" not in cfg["sim"]["mi355"] and "amp_forward_dynamics" not in cfg["sim"]["mi355"]          # (off by default)
    for key in ("forward_dynamics", "amp_forward_dynamics"):
        cfg = default_cfg(64, "cpu")
        cfg["sim"]["mi355"][key] = {"rhs": 2, "minv": True, "auto": True}
        validate_cfg(cfg)
        cfg["sim"]["mi355"][key] = True
        validate_cfg(cfg)
        for bad in ({"mass": True}, {"minv": 1}, {"rhs": 9}, "on"):
            cfg["sim"]["mi355"][key] = bad
            with pytest.raises(ValueError):
                validate_cfg(cfg)
    # TocabiAMPLower keeps its own key from the physics host
    src = open(os.path.join(ROOT, "isaacgymdyros_amd", "tocabi_amp_lower.py")).read()
    assert re.search(r'k not in \([^)]*"amp_forward_dynamics"[^)]*\)', src)
