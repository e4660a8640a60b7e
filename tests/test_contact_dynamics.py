"""The contact-consistent dynamics without a GPU (include/dyros_contact_dynamics.h, isaacgymdyros_amd/csrc/dw_contact.h, DESIGN.md section
26): the reference (tests/contact_dynamics_ref.py) against things that are not itself -- the chain's point velocities and accelerations, the
Schur path against the dense KKT solve, a fixed-base known answer; the per-env arithmetic -- compiled by g++ from the headers the HIP kernel
includes (tests/contact_dynamics_host.cpp) -- against the float64 reference under its measured tolerance; the outputs' exact properties; the
header, the Python binding and the built library; refusals; the kernel's resources; the cfg surface."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import body_states_ref as R
import contact_dynamics_ref as CR
import dynamics_ref as DR
import jacobians_ref as JR
from isaacgymdyros_amd import build, cbind
from isaacgymdyros_amd import contact_dynamics as CM
from isaacgymdyros_amd import forward_dynamics as FM
from isaacgymdyros_amd import jacobians as JM
from isaacgymdyros_amd.model import load_model
from test_body_states import TAKEN as TAKEN_BODIES          # noqa: F401
from test_gait_profile_abi import TAKEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dw_contact_dynamics.hip"
N = 37
F = np.float32
U = np.uint32
OUTS = CR.OUTS
BASE = (("base_link", (0.0, 0.0, 0.0)),)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------- 1. the reference against what is not itself
@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_reference_rows_are_the_chains_velocities_and_accelerations(K, vel_at_com):
    """jc nu is the contact points' velocity and the bodies' angular velocity of body_states_ref's chain (no Jacobian), and jc a + jdnu the
    points' classical acceleration and the bodies' angular acceleration of dynamics_ref.kinematics(a) for a seeded a, both within 1e-8 of the
    largest value (tests/test_forward_dynamics.py's bound)."""
    cs = CR.SETS[K]
    root, dof, _ms, _arm, acc = DR.seeded(64, 3 + vel_at_com)
    c = R.chain(root, dof, np.float64, vel_at_com)
    J, jd, r, m = CR.jc_of(c, cs, vel_at_com), CR.jdnu_of(c, dof, cs, vel_at_com), CR.arms(c, cs), CR.carriers(cs)
    vel = np.concatenate([c["vo"][:, m] + R.cross(c["w"][:, m], r), c["w"][:, m]], -1).reshape(64, -1)
    ev = np.abs(np.einsum("nrc,nc->nr", J, JR.nu(root, dof)) - vel).max()
    a = acc.astype(np.float64)
    om, al, xdd = (x[:, m] for x in DR.kinematics(c, dof, vel_at_com, a))
    want = np.concatenate([xdd + R.cross(al, r) + R.cross(om, R.cross(om, r)), al], -1).reshape(64, -1)
    ea = np.abs(np.einsum("nrc,nc->nr", J, a) + jd - want).max()
    print("K=%d: jc nu against the chain %.2e of %.1f; jc a + jdnu against kinematics(a) %.2e of %.0f" % (K, ev, np.abs(vel).max(), ea, np.abs(want).max()))
    assert ev <= 1e-8 * np.abs(vel).max() and ea <= 1e-8 * np.abs(want).max()


@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_reference_schur_path_is_the_dense_kkt_solve(K, vel_at_com):
    """The header's solve run in float64 against np.linalg.solve of the (39 + m)-square KKT matrix, within 1e-8 of the largest value; lambda
    lambda_inv = I; and the KKT residuals of the reference are at round-off: below 1000 ulp of (|KKT| |sol|)."""
    root, dof, ms, arm, _acc = DR.seeded(64, 5 + vel_at_com)
    rhs, sub = CR.rhs_of(root, dof, vel_at_com, ms, arm, 2, 7)
    gamma = CR.gamma_of(64, 6 * K, 9)
    want = CR.evaluate(root, dof, vel_at_com, ms, arm, CR.SETS[K], rhs, sub, gamma)
    got = CR.schur(root, dof, vel_at_com, ms, arm, CR.SETS[K], rhs, sub, gamma, dtype=np.float64)
    for k in OUTS:
        err, top = np.abs(got[k] - want[k]).max(), np.abs(want[k]).max()
        print("K=%d %s: the Schur path against the reference %.2e on values up to %.3g" % (K, k, err, top))
        assert err <= 1e-8 * top, k
    eye = np.abs(want["lambda"] @ want["lambda_inv"] - np.eye(6 * K)).max()
    sol = np.concatenate([want["accel"], want["force"]], -1)
    res = np.abs(np.einsum("nab,nrb->nra", want["KKT"], sol) - want["right"]).max()
    size = np.einsum("nab,nrb->nra", np.abs(want["KKT"]), np.abs(sol)).max()
    print("K=%d: lambda lambda_inv - I %.2e; KKT residual %.2e of %.3g; cond(A) up to %.3g" % (K, eye, res, size, np.linalg.cond(want["lambda_inv"]).max()))
    assert eye <= 1e-8 and res <= 1000 * 2.0 ** -52 * size


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_reference_one_contact_on_the_base_is_the_fixed_base_robot(vel_at_com):
    """The known answer: a contact on base_link at its origin prescribes the base's acceleration, accel[0:6] = X^-1 (gamma - jdnu) with X the
    base block of jc, and the joints move as a fixed-base robot's: accel[6:] = mm^-1 (b_j - M_jb accel[0:6]) with mm = M[6:, 6:] of
    jacobians_ref.  With origin velocities jdnu is exactly zero."""
    root, dof, ms, arm, _acc = DR.seeded(64, 11)
    rhs, sub = CR.rhs_of(root, dof, vel_at_com, ms, arm, 1, 13)
    gamma = CR.gamma_of(64, 6, 15)
    out = CR.evaluate(root, dof, vel_at_com, ms, arm, BASE, rhs, sub, gamma)
    M = JR.mass_matrix(R.chain(root, dof, np.float64, vel_at_com), vel_at_com, ms, arm)[0]
    b = rhs[:, 0].astype(np.float64) - sub.astype(np.float64)
    ab = np.linalg.solve(out["jc"][:, :, 0:6], (gamma.astype(np.float64) - out["jdnu"])[..., None])[..., 0]
    aj = np.linalg.solve(M[:, 6:, 6:], (b[:, 6:] - np.einsum("njb,nb->nj", M[:, 6:, 0:6], ab))[..., None])[..., 0]
    err, top = np.abs(out["accel"][:, 0] - np.concatenate([ab, aj], 1)).max(), np.abs(out["accel"]).max()
    print("fixed base, vel_at_com=%d: %.2e on accelerations up to %.0f" % (vel_at_com, err, top))
    assert err <= 1e-8 * top
    if not vel_at_com:
        assert (out["jdnu"] == 0).all()
    else:
        assert np.abs(out["jdnu"][:, 0:3]).max() > 0 and (out["jdnu"][:, 3:6] == 0).all()


# ---------------------------------------------------------------------------------------------- 2. the g++ build against float64
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/contact_dynamics_host.cpp")
    d = tmp_path_factory.mktemp("dwch")
    so, so_l = str(d / "libdwch.so"), str(d / "libdwlh.so")
    for out, src in ((so, "contact_dynamics_host.cpp"), (so_l, "forward_dynamics_host.cpp")):
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", out, os.path.join(ROOT, "tests", src)])
    lib = C.CDLL(so)
    lib.dwch_solve.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 9
    lib.dwch_pack_table.argtypes = [C.POINTER(JM.DwjModel), C.POINTER(CM.DwcContacts), C.c_void_p, C.c_char_p, C.c_int]
    lib.model = JM.model_struct(load_model())
    lib.tables = {}
    lib.fwd = C.CDLL(so_l)
    lib.fwd.dwlh_solve.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    return lib


def host_table(lib, contacts):
    key = tuple(contacts)
    if key not in lib.tables:
        table, err = np.zeros(CM.TABLE_WORDS, U), C.create_string_buffer(256)
        st = CM.contacts_struct(CR.ids_of(contacts), [p for _, p in contacts])
        assert lib.dwch_pack_table(C.byref(lib.model), C.byref(st), _p(table), err, 256) == 0, err.value
        lib.tables[key] = table
    return lib.tables[key]


def host_run(lib, contacts, root, dof, ms, arm, vel_at_com, rhs=None, sub=None, gamma=None, outs=OUTS, expect=0):
    """The outputs named, NaN-filled beforehand, as a dict (the others None)."""
    n, m = len(root), 6 * len(contacts)
    nrhs = 0 if rhs is None else rhs.shape[1]
    shape = {"jc": (n, m, 39), "jdnu": (n, m), "minv_jt": (n, m, 39), "lambda_inv": (n, m, m), "lambda": (n, m, m), "accel": (n, nrhs, 39), "force": (n, nrhs, m)}
    o = {k: np.full(shape[k], np.nan, F) if k in outs and (rhs is not None or k not in ("accel", "force")) else None for k in OUTS}
    rc = lib.dwch_solve(n, _p(host_table(lib, contacts)), _p(root), _p(dof), _p(ms), _p(arm), vel_at_com, _p(rhs), nrhs, _p(sub), _p(gamma), *[_p(o[k]) for k in OUTS])
    assert rc == expect
    return o


def same(a, b):
    return np.array_equal(a.view(U), b.view(U))


@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_host_build_against_float64(host, K, vel_at_com):
    """Every channel within 4 d of the float64 reference (accel and force: d scaled with the solution), every word written."""
    root, dof, ms, arm, _acc = DR.seeded(N, 11 + vel_at_com)
    rhs, sub = CR.rhs_of(root, dof, vel_at_com, ms, arm, 2, 17)
    gamma = CR.gamma_of(N, 6 * K, 19)
    o = host_run(host, CR.SETS[K], root, dof, ms, arm, vel_at_com, rhs, sub, gamma)
    assert all(np.isfinite(o[k]).all() for k in OUTS)
    ex = CR.excess(o, root, dof, ms, arm, vel_at_com, K, rhs, sub, gamma, report="host N=%d K=%d vel_at_com=%d" % (N, K, vel_at_com))
    assert len(ex) == len(CR.CHANNELS) and CR.within(ex), ex
    # nominal masses, no armature: another matrix, under the d measured for it (one case: the measurement takes its time)
    if not (vel_at_com == 1 and K == 2):
        return
    rhs, sub = CR.rhs_of(root, dof, vel_at_com, None, None, 1, 21)
    o = host_run(host, CR.SETS[K], root, dof, None, None, vel_at_com, rhs, sub, gamma)
    ex = CR.excess(o, root, dof, None, None, vel_at_com, K, rhs, sub, gamma, report="host, nominal masses, no armature")
    assert len(ex) == len(CR.CHANNELS) and CR.within(ex), ex


# ---------------------------------------------------------------------------------------------- 3. exact properties
@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("K", [2, 4])
def test_exact_properties(host, K, vel_at_com):
    cs, m = CR.SETS[K], 6 * K
    root, dof, ms, arm, _acc = DR.seeded(N, 21)
    R8 = CM.MAX_RHS
    rhs, sub = CR.rhs_of(root, dof, vel_at_com, ms, arm, R8, 23)
    gamma = CR.gamma_of(N, m, 25)
    o = host_run(host, cs, root, dof, ms, arm, vel_at_com, rhs, sub, gamma)
    assert all(np.isfinite(o[k]).all() for k in OUTS)
    # minv_jt[e, r] is dw_factor.h's solve of jc[e, r]: the bits of tests/forward_dynamics_host.cpp, six rows to a call
    table_l = np.ascontiguousarray(host_table(host, cs)[:FM.TABLE_WORDS])
    for i in range(K):
        x = np.full((N, 6, 39), np.nan, F)
        rows = np.ascontiguousarray(o["jc"][:, 6 * i:6 * i + 6])
        assert host.fwd.dwlh_solve(N, _p(table_l), _p(root), _p(dof), _p(ms), _p(arm), vel_at_com, _p(rows), 6, None, _p(x), None, None, None) == 0
        assert same(x, np.ascontiguousarray(o["minv_jt"][:, 6 * i:6 * i + 6])), i
    # lambda and lambda_inv: symmetric bit for bit
    for k in ("lambda", "lambda_inv"):
        assert same(o[k], np.ascontiguousarray(np.swapaxes(o[k], 1, 2))), k
    # 640 m out: the same bits
    far = root.copy()
    far[:, 0:2] += np.array([640.0, -640.0], F)
    of = host_run(host, cs, far, dof, ms, arm, vel_at_com, rhs, sub, gamma)
    assert all(same(of[k], o[k]) for k in OUTS)
    # jc: +0.0 off the path from the base to the carrying body, the identity blocks 1.0 and +0.0
    mask = np.repeat(JM.dof_mask(CR.ids_of(cs), load_model()), 6, 0)
    assert mask.shape == (m, 39) and (o["jc"].view(U)[:, ~mask] == 0).all()
    jc4 = o["jc"].reshape(N, K, 6, 39)
    one = np.float32(1.0).view(U)
    eye3 = np.where(np.eye(3, dtype=bool), one, U(0))
    assert (jc4[:, :, 0:3, 0:3].view(U) == eye3).all() and (jc4[:, :, 3:6, 3:6].view(U) == eye3).all() and (jc4[:, :, 3:6, 0:3].view(U) == 0).all()
    # gamma NULL equals a gamma of zeros; sub NULL equals a sub of zeros
    on = host_run(host, cs, root, dof, ms, arm, vel_at_com, rhs, sub, None, outs=("accel", "force"))
    oz = host_run(host, cs, root, dof, ms, arm, vel_at_com, rhs, sub, np.zeros((N, m), F), outs=("accel", "force"))
    assert same(on["accel"], oz["accel"]) and same(on["force"], oz["force"]) and not same(on["force"], o["force"])
    # b = 0, gamma = 0 and nu = 0 give zeros
    still_root, still_dof = root.copy(), dof.copy().reshape(N, 33, 2)
    still_root[:, 7:13] = 0
    still_dof[:, :, 1] = 0
    still_dof = np.ascontiguousarray(still_dof.reshape(dof.shape))
    os_ = host_run(host, cs, still_root, still_dof, ms, arm, vel_at_com, np.zeros((N, 2, 39), F), None, None)
    assert (os_["accel"] == 0).all() and (os_["force"] == 0).all() and (os_["jdnu"] == 0).all()
    # column r is the same bits at R = 1, 2 and 8
    for k in (1, 2):
        ok = host_run(host, cs, root, dof, ms, arm, vel_at_com, np.ascontiguousarray(rhs[:, :k]), sub, gamma, outs=("accel", "force"))
        assert same(ok["accel"], np.ascontiguousarray(o["accel"][:, :k])) and same(ok["force"], np.ascontiguousarray(o["force"][:, :k])), k
    last = host_run(host, cs, root, dof, ms, arm, vel_at_com, np.ascontiguousarray(rhs[:, R8 - 1:]), sub, gamma, outs=("accel", "force"))
    assert same(last["accel"][:, 0], o["accel"][:, R8 - 1]) and same(last["force"][:, 0], o["force"][:, R8 - 1])
    # the constraint holds: jc accel + jdnu = gamma within the allowances involved (float64 products of the float32 outputs)
    want = CR.evaluate(root, dof, vel_at_com, ms, arm, cs, rhs, sub, gamma)
    d = CR.measured(vel_at_com, K)
    res = np.einsum("nrc,nkc->nkr", o["jc"].astype(np.float64), o["accel"].astype(np.float64)) + o["jdnu"].astype(np.float64)[:, None] - gamma.astype(np.float64)[:, None]
    allow = (np.einsum("nrc,nkc->nkr", np.abs(want["jc"]), CR.allowance(want, vel_at_com, K, "accel"))
             + CR.FACTOR * max(d["jc_lin"], d["jc_ang"]) * np.abs(want["accel"]).sum(-1, keepdims=True) + CR.FACTOR * max(d["jdnu_lin"], d["jdnu_ang"]))
    print("K=%d: jc accel + jdnu - gamma: %.3f of the allowances involved" % (K, (np.abs(res) / allow).max()))
    assert (np.abs(res) <= allow).all()


def test_a_null_output_leaves_the_others_bits(host):
    cs = CR.SETS[2]
    root, dof, ms, arm, _acc = DR.seeded(N, 31)
    rhs, sub = CR.rhs_of(root, dof, 1, ms, arm, 3, 33)
    gamma = CR.gamma_of(N, 12, 35)
    full = host_run(host, cs, root, dof, ms, arm, 1, rhs, sub, gamma)
    for k in OUTS:
        needs = k in ("accel", "force")
        one = host_run(host, cs, root, dof, ms, arm, 1, *((rhs, sub, gamma) if needs else (None, None, None)), outs=(k,))
        assert same(one[k], full[k]) and all(one[j] is None for j in OUTS if j != k), k
        rest = host_run(host, cs, root, dof, ms, arm, 1, rhs, sub, gamma, outs=tuple(j for j in OUTS if j != k))
        assert rest[k] is None and all(same(rest[j], full[j]) for j in OUTS if j != k), k


def test_non_finite_inputs_stay_in_their_env(host):
    cs = CR.SETS[2]
    root, dof, ms, arm, _acc = DR.seeded(6, 41)
    rhs, sub = CR.rhs_of(root, dof, 1, ms, arm, 2, 43)
    gamma = CR.gamma_of(6, 12, 45)
    o0 = host_run(host, cs, root, dof, ms, arm, 1, rhs, sub, gamma)
    root[2, 4], dof[3, 4, 0], rhs[5, 1, 7] = np.nan, np.inf, np.nan          # (DoF 4 drives moving body 5, on the left foot's path)
    o = host_run(host, cs, root, dof, ms, arm, 1, rhs, sub, gamma)
    for k in OUTS:
        assert same(o[k][[0, 1, 4]], o0[k][[0, 1, 4]]), k
        assert np.isnan(o[k][2]).any() and np.isnan(o[k][3]).any(), k
    # a NaN in one right-hand side reaches that column of accel and force alone
    for k in ("accel", "force"):
        assert np.isnan(o[k][5, 1]).any() and same(o[k][5, 0], o0[k][5, 0]), k
    assert all(same(o[k][5], o0[k][5]) for k in OUTS if k not in ("accel", "force"))


# ---------------------------------------------------------------------------------------------- 4. the ABI
@pytest.fixture(scope="module")
def api():
    return cbind.declare(C.CDLL(build.build()), "dyros_contact_dynamics.h", "dwc_")


@pytest.mark.parametrize("check", ["prototypes", "layouts"])
def test_header_python_and_library_agree(check, tmp_path):
    import test_cbind as TC
    if check == "prototypes":
        TC.test_ctypes_prototypes_match_the_header("dyros_contact_dynamics.h", "dwc_", "contact_dynamics", C.CDLL(build.build()))
    else:
        TC.test_struct_layouts_match_the_host_compiler("dyros_contact_dynamics.h", "dwc_", "contact_dynamics", tmp_path)
    assert sorted(CM.EXPORTS) == ["abi_version", "last_error", "pack_table", "solve"]
    assert dict(build.SOURCES)[SRC] == ["-ffp-contract=off"] and "dw_contact.h" in build.HEADERS
    K, KL = CM.K, FM.K
    assert K["DWC_ABI_VERSION"] == 1 and (K["DWC_NV"], K["DWC_MAX_CONTACTS"], K["DWC_ROWS"], K["DWC_MAX_ROWS"], K["DWC_MAX_RHS"]) == (39, 4, 6, 24, 8)
    for name in ("NUM_BODIES", "NUM_DOF", "NV", "MAX_RHS"):
        assert K["DWC_" + name] == KL["DWL_" + name]
    assert K["DWC_T_K"] == KL["DWL_TABLE_WORDS"] and K["DWC_T_CONTACT"] == K["DWC_T_K"] + 1 and K["DWC_TABLE_WORDS"] == K["DWC_T_CONTACT"] + 16 + 3
    assert K["DWC_TABLE_WORDS"] % 4 == 0 and K["DWC_GROUP"] * K["DWC_LANES"] <= 1024 and K["DWC_LANES"] == 64
    assert CM.DEFAULTS == {"contacts": [{"body": "L_Foot_Link", "pos": [0.0, 0.0, -0.09]}, {"body": "R_Foot_Link", "pos": [0.0, 0.0, -0.09]}], "rhs": 1,
                           "jacobian": True, "lambda": True, "lambda_inv": False, "minv_jt": False, "armature": True, "auto": False}
    # the older headers are untouched
    assert KL["DWL_ABI_VERSION"] == 1 and JM.K["DWJ_ABI_VERSION"] == 1 and cbind.constants("dyros_dynamics.h", "dwn_")["DWN_ABI_VERSION"] == 1


def test_the_library_and_the_host_build_pack_the_same_table(host, api):
    lapi = cbind.declare(C.CDLL(build.build()), "dyros_forward_dynamics.h", "dwl_")
    model = load_model()
    for K in (1, 2, 4):
        cs = CR.SETS[K]
        t = CM.pack_table(api, model, CR.ids_of(cs), [p for _, p in cs])
        assert t.dtype == U and t.shape == (CM.TABLE_WORDS,) and np.array_equal(t, host_table(host, cs))
        assert np.array_equal(t[:CM.K["DWC_T_K"]], FM.pack_table(lapi, model)) and t[CM.K["DWC_T_K"]] == K
        words = t[CM.K["DWC_T_CONTACT"]:CM.K["DWC_T_CONTACT"] + 16].reshape(4, 4)
        assert list(words[:K, 0]) == CR.carriers(cs) and np.array_equal(words[:K, 1:].view(F), np.array([p for _, p in cs], F))
        assert (words[K:] == 0).all() and (t[-3:] == 0).all()
    # a jointless body stands for the moving body it is welded to
    a, b = (CM.pack_table(api, model, [g], [[0.1, 0.0, 0.0]]) for g in (6, 8))
    assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_pack_table_refusals(api):
    model = load_model()
    feet, pos = [8, 16], [[0, 0, -0.09]] * 2
    bad = ((([], []), "count must be in 1..DWC_MAX_CONTACTS"), (([1, 2, 3, 4, 5], [[0, 0, 0]] * 5), "count must be in 1..DWC_MAX_CONTACTS"),
           (([8, 38], pos), "a body id is outside 0..37"), (([-1], pos[:1]), "a body id is outside 0..37"),
           ((feet, [[0, 0, -0.09], [0, float("nan"), 0]]), "pos is not finite"), ((feet, [[float("inf"), 0, 0], [0, 0, 0]]), "pos is not finite"),
           (([8, 6], pos), "two contacts on one moving body"), (([7, 16, 8], pos + pos[:1]), "two contacts on one moving body"), (([0, 0], pos), "two contacts on one moving body"))
    for (ids, p), msg in bad:
        with pytest.raises(cbind.DyrosWalkLibraryError, match="dwc_pack_table: " + msg):
            CM.pack_table(api, model, ids, p)
    # it refuses what dwl_pack_table refuses, under its own name
    d = {k: np.array(v) for k, v in model.d.items() if k in ("mv_parent", "mv_pos", "mv_rot0", "mv_axis", "body_moving", "inert_gym", "inert_mv", "inert_mass",
                                                             "inert_com", "inert_I")}
    d["mv_parent"][5] = 6
    with pytest.raises(cbind.DyrosWalkLibraryError, match="dwc_pack_table: a child precedes its parent"):
        CM.pack_table(api, d, feet, pos)
    d["mv_parent"][5] = model.d["mv_parent"][5]
    d["inert_I"][9][1][1] = float("nan")
    with pytest.raises(cbind.DyrosWalkLibraryError, match="dwc_pack_table: inert_I is not finite"):
        CM.pack_table(api, d, feet, pos)
    t = np.zeros(CM.TABLE_WORDS, U)
    assert api["pack_table"](None, C.byref(CM.contacts_struct(feet, pos)), t.ctypes.data) == -1 and b"a pointer is missing" in api["last_error"]()
    assert api["pack_table"](C.byref(JM.model_struct(model)), None, t.ctypes.data) == -1 and b"a pointer is missing" in api["last_error"]()


def test_refusals_happen_before_any_launch(api):
    """Every buffer is NULL or a host address here: a launch would fault, a refusal returns -1 with its message."""
    one = C.c_void_p(16)
    ok = lambda **kw: tuple(dict(dict(n=8, table=one, root=one, dof=one, ms=None, arm=None, vac=0, rhs=one, nrhs=1, sub=None, gamma=None, jc=None,          # noqa: E731
                                      jdnu=None, minv_jt=None, lambda_inv=None, lam=None, accel=one, force=one, stream=None), **kw).values())
    for args, msg in ((ok(n=0), b"num_envs"), (ok(n=-3), b"num_envs"), (ok(n=1 << 30), b"num_envs"),
                      (ok(table=None), b"a buffer is missing"), (ok(root=None), b"a buffer is missing"), (ok(dof=None), b"a buffer is missing"),
                      (ok(table=C.c_void_p(8)), b"16-byte aligned"),
                      (ok(accel=None, force=None), b"rhs needs accel or force"), (ok(accel=None, force=None, jc=one), b"rhs needs accel or force"),
                      (ok(rhs=None), b"accel and force need rhs"), (ok(rhs=None, force=None), b"accel and force need rhs"),
                      (ok(rhs=None, accel=None, lam=one), b"accel and force need rhs"),
                      (ok(rhs=None, accel=None, force=None, sub=one, jc=one), b"sub needs rhs"),
                      (ok(rhs=None, accel=None, force=None, gamma=one, jc=one), b"gamma needs rhs"),
                      (ok(nrhs=0), b"nrhs"), (ok(nrhs=-1), b"nrhs"), (ok(nrhs=CM.MAX_RHS + 1), b"nrhs"),
                      (ok(rhs=None, accel=None, force=None), b"no output"), (ok(rhs=None, accel=None, force=None, nrhs=0), b"no output")):
        assert api["solve"](*args) == -1 and msg in api["last_error"]() and b"dwc_solve" in api["last_error"](), (args, api["last_error"]())


# ---------------------------------------------------------------------------------------------- 6. the kernel's resources
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
    assert "dwc_k_solve" in names[0]
    for n, s, l in zip(names, scratch, lds):
        assert "dwc_k_" in n and s == 0 and l <= 65536, (n, s, l)
        assert not any(x in n for x in tuple(TAKEN) + tuple(TAKEN_BODIES) + ("dwg_k_", "dwb_k_", "dwf_k_", "dwj_k_", "dwn_k_", "dwl_k_")), n
        assert not any(x in n for x in ("k_mlp", "k_wgrad", "k_policy", "k_adam", "k_grad_stats", "k_finish", "k_gae", "k_roll_pre", "k_roll_post", "k_loss",
                                        "k_relu_bwd", "k_bias_relu", "k_stage_obs", "k_retile", "dw_k_amp", "dw_k_newwalk", "dw_k_body_positions")), n
    print("dwc_k_solve: LDS %d bytes per workgroup" % lds[0])


# ---------------------------------------------------------------------------------------------- 7. the Python surface
def test_cfg_spec():
    assert CM.resolve(None) is None and CM.resolve(False) is None
    full = CM.resolve(True)
    assert full == CM.resolve({}) and {k: full[k] for k in CM.DEFAULTS} == CM.DEFAULTS and full["ids"] == [8, 16] and full["pos"] == [[0.0, 0.0, -0.09]] * 2
    s = CM.resolve({"contacts": [{"body": "base_link"}, {"body": 27, "pos": [0.1, 0, 0]}], "rhs": 3, "jacobian": False, "lambda": False, "lambda_inv": True,
                    "minv_jt": True, "auto": True, "armature": False})
    assert s["ids"] == [0, 27] and s["pos"] == [[0.0, 0.0, 0.0], [0.1, 0.0, 0.0]] and s["rhs"] == 3 and s["lambda_inv"] and s["minv_jt"] and s["auto"]
    assert not (s["jacobian"] or s["lambda"] or s["armature"])
    assert CM.resolve({"rhs": CM.MAX_RHS})["rhs"] == CM.MAX_RHS
    foot = {"body": "L_Foot_Link"}
    for bad in (1, "on", ["lambda"], {"h": True}, {"jacobian": 1}, {"lambda": None}, {"lambda_inv": "yes"}, {"minv_jt": 0}, {"armature": 1.0}, {"auto": "no"},
                {"rhs": 0}, {"rhs": CM.MAX_RHS + 1}, {"rhs": True}, {"rhs": 2.0}, {"rhs": "1"}, {1: True},
                {"contacts": []}, {"contacts": "L_Foot_Link"}, {"contacts": [foot] * 5}, {"contacts": ["L_Foot_Link"]}, {"contacts": [{"pos": [0, 0, 0]}]},
                {"contacts": [{"body": "no_such_link"}]}, {"contacts": [{"body": 38}]}, {"contacts": [{"body": True}]}, {"contacts": [{"body": 8, "quat": [0, 0, 0, 1]}]},
                {"contacts": [{"body": 8, "pos": [0, 0]}]}, {"contacts": [{"body": 8, "pos": [0, 0, float("nan")]}]}, {"contacts": [{"body": 8, "pos": "abc"}]},
                {"contacts": [foot, {"body": "L_AnkleRoll_Link"}]}, {"contacts": [foot, {"body": 7}]}):
        with pytest.raises(ValueError):
            CM.resolve(bad)
    from isaacgymdyros_amd.config import default_cfg, validate_cfg
    cfg = default_cfg(64, "cpu")
    assert "contact_dynamics" not in cfg["sim"]["mi355"] and "amp_contact_dynamics" not in cfg["sim"]["mi355"]          # (off by default)
    for key in ("contact_dynamics", "amp_contact_dynamics"):
        cfg = default_cfg(64, "cpu")
        cfg["sim"]["mi355"][key] = {"rhs": 2, "minv_jt": True, "auto": True, "contacts": [foot]}
        validate_cfg(cfg)
        cfg["sim"]["mi355"][key] = True
        validate_cfg(cfg)
        for bad in ({"mass": True}, {"lambda": 1}, {"rhs": 9}, "on", {"contacts": [foot, foot]}):
            cfg["sim"]["mi355"][key] = bad
            with pytest.raises(ValueError):
                validate_cfg(cfg)
    # TocabiAMPLower keeps its own key from the physics host
    src = open(os.path.join(ROOT, "isaacgymdyros_amd", "tocabi_amp_lower.py")).read()
    assert re.search(r'k not in \([^)]*"amp_contact_dynamics"[^)]*\)', src)
