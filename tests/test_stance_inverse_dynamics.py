"""The stance inverse dynamics without a GPU (include/dyros_stance_inverse_dynamics.h, isaacgymdyros_amd/csrc/dw_stance_inverse.h, DESIGN.md
section 28): the reference (tests/stance_inverse_dynamics_ref.py) against what it is not itself -- section 27's reference on the contact
subset; the per-env arithmetic -- compiled by g++ from the headers the HIP kernel includes (tests/contact_inverse_dynamics_host.cpp) -- against
the float64 reference under its measured tolerance; the exact properties against section 27's plain row-ordered sums, stated in that g++
build only; the standing pose; stance_from_phase's windows; the header, the Python binding and the built library; refusals; the kernel's
resources; the cfg surface."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import contact_dynamics_ref as CR
import contact_inverse_dynamics_ref as IR
import dynamics_ref as DR
import inverse_dynamics_resources as RES
import stance_inverse_dynamics_ref as SR
from isaacgymdyros_amd import build, cbind
from isaacgymdyros_amd import contact_dynamics as CM
from isaacgymdyros_amd import contact_inverse_dynamics as IM
from isaacgymdyros_amd import jacobians as JM
from isaacgymdyros_amd import stance_inverse_dynamics as SM
from isaacgymdyros_amd.model import load_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dw_contact_inverse.hip"          # (one unit holds dwi_k_solve and dwk_k_solve)
HEADER = "dyros_stance_inverse_dynamics.h"
N = 37
F, U = np.float32, np.uint32
OUTS, IOUTS = SR.OUTS, IR.OUTS
GRAV = DR.GRAVITY
W10 = IR.MOMENTS_10
WEIGHTS = (None, W10)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------- 1. the reference against what is not itself
@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("K", [2, 4])
def test_reference_is_section_27s_on_the_contact_subset(K, vel_at_com):
    """Env by env, for every stance pattern: force and tau_joint are contact_inverse_dynamics_ref.evaluate's on the env's contact subset with
    that subset's weights and f_ref (called here per env, not per pattern), the inactive rows zero; the base rows are carried (base_residual
    <= 1e-8 of r) unless the env is in flight, where it is r[0:6]; contact_accel and tau_full are section 27's for all contacts; the margins
    agree with a plain matrix restatement (R' f, R' m, the moment moved to the sole centre by a cross product)."""
    cs, n, m = SR.SETS[K], 2 << K, 6 * K
    root, dof, ms, arm, acc = DR.seeded(n, 3 + vel_at_com)
    fr, st = IR.fref_of(n, m, 5), SR.stance_cycle(n, K, 1)
    w = [[1.0, 1.0, 1.0, 10.0, 10.0, 10.0], [10.0] * 6, [2.0] * 6, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]][:K]
    o = SR.evaluate(root, dof, vel_at_com, ms, arm, cs, st, acc, w, fr, mu=0.7)
    full = IR.evaluate(root, dof, vel_at_com, ms, arm, cs, acc, w, fr)
    assert np.array_equal(o["contact_accel"], full["contact_accel"]) and np.array_equal(o["tau_full"], full["tau_full"])
    c = SR.R.chain(root, dof, np.float64, vel_at_com)
    Rb = c["R"][:, CR.carriers(cs)]
    so, pos = SR.soles_of(cs).astype(np.float64), np.array([p for _, p in cs], F).astype(np.float64)
    for e in range(n):
        S = [i for i in range(K) if st[e, i]]
        rows = [6 * i + k for i in S for k in range(6)]
        off = [r for r in range(m) if r not in rows]
        assert (o["force"][e, off] == 0).all() and (o["margins"][e].reshape(K, 4)[[i for i in range(K) if i not in S]] == 0).all()
        if not S:
            assert (np.array_equal(o["tau_joint"][e], o["tau_full"][e, 6:]) and np.array_equal(o["base_residual"][e], o["tau_full"][e, 0:6])
                    and o["feasible"][e] == 0)
            continue
        one = IR.evaluate(root[e:e + 1], dof[e:e + 1], vel_at_com, ms[e:e + 1], arm[e:e + 1], tuple(cs[i] for i in S), acc[e:e + 1], [w[i] for i in S],
                          fr[e:e + 1][:, rows])
        assert np.abs(one["force"][0] - o["force"][e, rows]).max() <= 1e-9 * np.abs(one["force"]).max()
        assert np.abs(one["tau_joint"][0] - o["tau_joint"][e]).max() <= 1e-9 * np.abs(one["tau_joint"]).max()
        assert np.abs(o["base_residual"][e]).max() <= 1e-8 * np.abs(o["tau_full"][e, 0:6]).max()
        for i in S:
            f, mo = Rb[e, i].T @ o["force"][e, 6 * i:6 * i + 3], Rb[e, i].T @ o["force"][e, 6 * i + 3:6 * i + 6]
            ms_ = mo - np.cross(so[i, 0:3] - pos[i], f)
            want = np.array([f[2], float(F(0.7)) * f[2] - np.hypot(f[0], f[1]), so[i, 3] * f[2] - abs(ms_[1]), so[i, 4] * f[2] - abs(ms_[0])])
            assert np.abs(want - o["margins"][e, i]).max() <= 1e-9 * max(1.0, np.abs(o["force"][e]).max())
        assert o["feasible"][e] == int((o["margins"][e, S] >= 0).all())
    # an all-ones stance is section 27
    ones = SR.evaluate(root, dof, vel_at_com, ms, arm, cs, None, acc, w, fr)
    assert np.abs(ones["force"] - full["force"]).max() <= 1e-9 * np.abs(full["force"]).max() and np.array_equal(ones["stance"], np.ones((n, K), np.uint8))


# ---------------------------------------------------------------------------------------------- 2. the g++ builds
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/contact_inverse_dynamics_host.cpp")
    so = str(tmp_path_factory.mktemp("dwkh") / "libdwkh.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, os.path.join(ROOT, "tests", "contact_inverse_dynamics_host.cpp")])
    lib = C.CDLL(so)
    lib.dwkh_solve.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_float] * 3 + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 7
    lib.dwkh_pack_table.argtypes = [C.POINTER(JM.DwjModel), C.POINTER(CM.DwcContacts), C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_char_p, C.c_int]
    lib.model = JM.model_struct(load_model())
    lib.tables = {}
    lib.inv = lib          # (dwih_solve: section 27's plain row-ordered sums, stated in the host file only)
    lib.inv.dwih_solve.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_float] * 3 + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 4
    lib.inv.dwih_pack_table.argtypes = [C.POINTER(JM.DwjModel), C.POINTER(CM.DwcContacts), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    return lib


def flat_weights(weights, K):
    return None if weights is None else (np.tile(np.asarray(weights, F), K) if np.asarray(weights).size == 6 else np.asarray(weights, F).reshape(-1))


def host_table(lib, contacts, weights=None, soles=None, mu=1.0):
    so = SR.soles_of(contacts) if soles is None else np.asarray(soles, F)
    key = (tuple(contacts), None if weights is None else tuple(np.asarray(weights, F).reshape(-1)), tuple(so.reshape(-1)), float(mu))
    if key not in lib.tables:
        table, err = np.zeros(SM.TABLE_WORDS, U), C.create_string_buffer(256)
        st = CM.contacts_struct(CR.ids_of(contacts), [p for _, p in contacts])
        assert lib.dwkh_pack_table(C.byref(lib.model), C.byref(st), _p(flat_weights(weights, len(contacts))), _p(np.ascontiguousarray(so)), mu, _p(table), err, 256) == 0, err.value
        lib.tables[key] = table
    return lib.tables[key]


def shapes(n, K):
    return {"tau_joint": (n, 33), "force": (n, 6 * K), "contact_accel": (n, 6 * K), "tau_full": (n, 39), "base_residual": (n, 6), "margins": (n, K, 4), "feasible": (n,)}


def host_run(lib, contacts, root, dof, ms, arm, vel_at_com, stance=None, accel=None, f_ref=None, weights=None, outs=OUTS, g=GRAV, soles=None, mu=1.0):
    """The outputs named, NaN-filled (feasible: 255) beforehand, as a dict (the others None)."""
    n, K = len(root), len(contacts)
    o = {k: (np.full(s, 255, np.uint8) if k == "feasible" else np.full(s, np.nan, F)) if k in outs else None for k, s in shapes(n, K).items()}
    st = None if stance is None else np.ascontiguousarray(stance, np.uint8)
    rc = lib.dwkh_solve(n, _p(host_table(lib, contacts, weights, soles, mu)), _p(root), _p(dof), _p(ms), _p(arm), g[0], g[1], g[2], _p(accel), _p(f_ref), _p(st),
                        vel_at_com, *[_p(o[k]) for k in OUTS])
    assert rc == 0
    return o


def inv_run(lib, contacts, root, dof, ms, arm, vel_at_com, accel=None, f_ref=None, weights=None, g=GRAV):
    """The g++ build of section 27's plain row-ordered arithmetic (tests/contact_inverse_dynamics_host.cpp's dwih_solve)."""
    n, m = len(root), 6 * len(contacts)
    table, err = np.zeros(IM.TABLE_WORDS, U), C.create_string_buffer(256)
    st = CM.contacts_struct(CR.ids_of(contacts), [p for _, p in contacts])
    assert lib.inv.dwih_pack_table(C.byref(lib.model), C.byref(st), _p(flat_weights(weights, len(contacts))), _p(table), err, 256) == 0, err.value
    o = {k: np.full(s, np.nan, F) for k, s in (("tau_joint", (n, 33)), ("force", (n, m)), ("contact_accel", (n, m)), ("tau_full", (n, 39)))}
    assert lib.inv.dwih_solve(n, _p(table), _p(root), _p(dof), _p(ms), _p(arm), g[0], g[1], g[2], _p(accel), _p(f_ref), vel_at_com, *[_p(o[k]) for k in IOUTS]) == 0
    return o


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(U if a.dtype == F else np.uint8), np.ascontiguousarray(b).view(U if b.dtype == F else np.uint8))


def check_feasible(got, want, allow):
    """feasible is the reference's wherever no active margin of the reference is within its allowance of zero; 0 in flight."""
    clear = (~(want["stance"][:, :, None] != 0) | (np.abs(want["margins"]) > allow)).all((1, 2))
    assert clear.any() and np.array_equal(got[clear], want["feasible"][clear]) and (got[want["stance"].sum(1) == 0] == 0).all() and set(np.unique(got)) <= {0, 1}


@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("K", [2, 4])
def test_host_build_against_float64(host, K, vel_at_com):
    """Every channel within 4 d of the float64 reference, every word written, no state left out: K = 2 with every stance pattern, K = 4 with a
    seeded mix; unit weights and moments weighted 10 x, with and without f_ref."""
    cs = SR.SETS[K]
    root, dof, ms, arm, acc = DR.seeded(N, 11 + vel_at_com)
    st = SR.stance_cycle(N, K) if K == 2 else SR.stance_mix(N, K, 17)
    for w in WEIGHTS:
        for fr in (None, IR.fref_of(N, 6 * K, 13)):
            o = host_run(host, cs, root, dof, ms, arm, vel_at_com, st, acc, fr, w)
            assert all(np.isfinite(o[k]).all() for k in OUTS)
            want = SR.evaluate(root, dof, vel_at_com, ms, arm, cs, st, acc, w, fr)
            ex = SR.excess(o, want, vel_at_com, K, w, fr is not None,
                           report="host N=%d K=%d vel_at_com=%d weights %s f_ref %s" % (N, K, vel_at_com, "unit" if w is None else "10 x", fr is not None))
            assert len(ex) == len(SR.CHANNELS) and SR.within(ex), ex
            check_feasible(o["feasible"], want, SR.allowance(want, vel_at_com, K, "margins", w, fr is not None))


# ---------------------------------------------------------------------------------------------- 3. exact properties
@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_exact_properties(host, vel_at_com):
    v = vel_at_com
    root, dof, ms, arm, acc = DR.seeded(N, 23)
    for K in (2, 4):
        cs, m = SR.SETS[K], 6 * K
        fr = IR.fref_of(N, m, 25)
        # an all-ones or NULL stance: dwi_solve's bits in all four outputs, with weights and f_ref
        inv = inv_run(host, cs, root, dof, ms, arm, v, acc, fr, W10)
        for st in (None, np.ones((N, K), np.uint8), np.full((N, K), 255, np.uint8), SR.stance_cycle(N, K) + 1):
            o = host_run(host, cs, root, dof, ms, arm, v, st, acc, fr, W10)
            assert all(same(o[k], inv[k]) for k in IOUTS) and np.isfinite(o["margins"]).all() and np.isfinite(o["base_residual"]).all()
        # one active contact i with unit weights: in its rows and in tau_joint the bits of dwi_solve on the one-contact table of contact i,
        # with f_ref that contact's rows or NULL; the other rows +0.0 and their f_ref (NaN here) not read
        for i in range(K):
            st = np.zeros((N, K), np.uint8)
            st[:, i] = 1
            for ref in (fr, None):
                bad = None if ref is None else np.full((N, m), np.nan, F)
                if ref is not None:
                    bad[:, 6 * i:6 * i + 6] = ref[:, 6 * i:6 * i + 6]
                o = host_run(host, cs, root, dof, ms, arm, v, st, acc, bad)
                one = inv_run(host, cs[i:i + 1], root, dof, ms, arm, v, acc, None if ref is None else np.ascontiguousarray(ref[:, 6 * i:6 * i + 6]))
                assert same(o["force"][:, 6 * i:6 * i + 6], one["force"]) and same(o["tau_joint"], one["tau_joint"]), (K, i)
                rest = np.delete(o["force"], np.s_[6 * i:6 * i + 6], 1)
                assert (rest.view(U) == 0).all() and (np.delete(o["margins"], i, 1).view(U) == 0).all()
                assert same(o["contact_accel"], inv["contact_accel"]) and same(o["tau_full"], inv["tau_full"])
        # flight: nothing is factored, no word is NaN; force +0.0, tau_joint = tau_full[6:], base_residual = tau_full[0:6], bit for bit
        o = host_run(host, cs, root, dof, ms, arm, v, np.zeros((N, K), np.uint8), acc, np.full((N, m), np.nan, F), W10)
        assert all(np.isfinite(o[k]).all() for k in OUTS)
        assert (o["force"].view(U) == 0).all() and (o["margins"].view(U) == 0).all() and (o["feasible"] == 0).all()
        assert same(o["tau_joint"], np.ascontiguousarray(o["tau_full"][:, 6:])) and same(o["base_residual"], np.ascontiguousarray(o["tau_full"][:, 0:6]))
        assert same(o["tau_full"], inv["tau_full"]) and same(o["contact_accel"], inv["contact_accel"])
        # a mixed batch: every env has the bits it has alone, a NULL output leaves the others' bits, 640 m out is the same bits
        st = SR.stance_cycle(N, K, 3)
        o = host_run(host, cs, root, dof, ms, arm, v, st, acc, fr, W10)
        for e in (0, 1, 5, N - 1):
            alone = host_run(host, cs, root[e:e + 1], dof[e:e + 1], ms[e:e + 1], arm[e:e + 1], v, st[e:e + 1], acc[e:e + 1], fr[e:e + 1], W10)
            assert all(same(alone[k][0], o[k][e]) for k in OUTS), e
        for k in OUTS:
            one = host_run(host, cs, root, dof, ms, arm, v, st, acc, fr, W10, outs=(k,))
            assert same(one[k], o[k]) and all(one[j] is None for j in OUTS if j != k), k
            rest = host_run(host, cs, root, dof, ms, arm, v, st, acc, fr, W10, outs=tuple(j for j in OUTS if j != k))
            assert rest[k] is None and all(same(rest[j], o[j]) for j in OUTS if j != k), k
        far = root.copy()
        far[:, 0:2] += np.array([640.0, -640.0], F)
        of = host_run(host, cs, far, dof, ms, arm, v, st, acc, fr, W10)
        assert all(same(of[k], o[k]) for k in OUTS)
        # feasible is the margins' sign, word for word
        want = (st.sum(1) > 0) & ((o["margins"] >= 0) | (st[:, :, None] == 0)).all((1, 2))
        assert np.array_equal(o["feasible"], want.astype(np.uint8))
        # base_residual is rounding where the stance is not empty: within 4 d
        ref = SR.evaluate(root, dof, v, ms, arm, cs, st, acc, W10, fr)
        assert (np.abs(o["base_residual"] - ref["base_residual"]) <= SR.allowance(ref, v, K, "base_residual", W10, True)).all()


def test_non_finite_inputs_stay_in_their_env(host):
    cs = SR.SETS[2]
    root, dof, ms, arm, acc = DR.seeded(8, 41)
    fr, st = IR.fref_of(8, 12, 43), SR.stance_cycle(8, 2, 1)
    o0 = host_run(host, cs, root, dof, ms, arm, 1, st, acc, fr)
    root[2, 4], dof[4, 4, 0], acc[5, 7] = np.nan, np.inf, np.nan          # (DoF 4 drives moving body 5, on the left foot's path; envs 4 and 5 stand on it)
    o = host_run(host, cs, root, dof, ms, arm, 1, st, acc, fr)
    for k in OUTS:
        assert same(o[k][[0, 1, 3, 6, 7]], o0[k][[0, 1, 3, 6, 7]]), k
    assert all(np.isnan(o[k][e]).any() for k in ("tau_joint", "force", "tau_full", "margins") for e in (2, 4)) and np.isnan(o["tau_joint"][5]).any()
    assert (o["feasible"][[2, 4]] == 0).all()          # (a NaN margin is not >= 0)


# ---------------------------------------------------------------------------------------------- 4. the standing pose
def standing(n=1):
    from isaacgymdyros_amd.task_constants import INITIAL_DOF_POS
    root = np.zeros((n, 13), F)
    root[:, 2], root[:, 6] = 0.93, 1.0
    dof = np.zeros((n, 33, 2), F)
    dof[:, :, 0] = np.asarray(INITIAL_DOF_POS, F)
    return root, np.ascontiguousarray(dof.reshape(n, 66))


def test_standing_pose(host):
    """INITIAL_DOF_POS, identity root, nu = a = 0, unit weights.  Both feet: every margin > 0, feasible.  One foot: about 1025 N on it, and the
    centre of pressure 9.8 cm (left) and 10.7 cm (right) to the side of a sole 8.5 cm wide: the fourth margin < 0 (the float64 reference:
    -13.4 and -22.5 N m, far from zero; the centre of mass of this pose lies 4.5 mm to the left of the middle, body_states_ref.com, which
    is the two figures' difference: 1025 N x 2 x 4.5 mm), the other three > 0, not feasible."""
    root, dof = standing(3)
    st = np.array([[1, 1], [1, 0], [0, 1]], np.uint8)
    cs = SR.SETS[2]
    o = host_run(host, cs, root, dof, None, None, 0, st)
    ref = SR.evaluate(root, dof, 0, None, None, cs, st)
    print("standing: force z", o["force"].reshape(3, 2, 6)[:, :, 2], "margins", o["margins"], "reference", ref["margins"])
    for x in (o, ref):
        mg = x["margins"]
        assert (mg[0] > 0).all() and x["feasible"][0] == 1
        for e, i in ((1, 0), (2, 1)):
            assert mg[e, i, 3] < -10.0 and (mg[e, i, 0:3] > 0).all() and x["feasible"][e] == 0 and (mg[e, 1 - i] == 0).all()
            assert 1000.0 < x["force"].reshape(3, 2, 6)[e, i, 2] < 1050.0
        assert 480.0 < x["force"].reshape(3, 2, 6)[0, 0, 2] < 540.0
    assert sorted(round(float(v), 1) for v in ref["margins"][[1, 2], [0, 1], 3]) == [-22.5, -13.4]


# ---------------------------------------------------------------------------------------------- 5. stance_from_phase's windows
def test_phase_windows():
    """The reward's windows of csrc/dw_gait.h at their edges: 300 <= idx < 1500 right foot only, 2100 <= idx < 3300 left foot only."""
    idx = np.array([0, 299, 300, 1499, 1500, 2099, 2100, 3299, 3300, 3599])
    left, right = SM.phase_stance(idx)
    assert left.tolist() == [True, True, False, False, True, True, True, True, True, True]
    assert right.tolist() == [True, True, True, True, True, True, False, False, True, True]
    src = open(os.path.join(build.CSRC, "dw_gait.h")).read()
    assert "300 <= idx && idx < 1500) return DWG_WIN_RSSP" in src and "2100 <= idx && idx < 3300) return DWG_WIN_LSSP" in src
    assert (SM.RSSP, SM.LSSP) == ((300, 1500), (2100, 3300))
    import torch
    l, r = SM.phase_stance(torch.from_numpy(idx).to(torch.int32))          # (the env's path: torch ops on the int32 view)
    assert l.tolist() == left.tolist() and r.tolist() == right.tolist()


# ---------------------------------------------------------------------------------------------- 6. the ABI
@pytest.fixture(scope="module")
def api():
    return cbind.declare(C.CDLL(build.build()), HEADER, "dwk_")


@pytest.mark.parametrize("check", ["prototypes", "layouts"])
def test_header_python_and_library_agree(check, tmp_path):
    import test_cbind as TC
    if check == "prototypes":
        TC.test_ctypes_prototypes_match_the_header(HEADER, "dwk_", "stance_inverse_dynamics", C.CDLL(build.build()))
    else:
        TC.test_struct_layouts_match_the_host_compiler(HEADER, "dwk_", "stance_inverse_dynamics", tmp_path)
    assert sorted(SM.EXPORTS) == ["abi_version", "last_error", "pack_table", "solve"]
    assert dict(build.SOURCES)[SRC] == ["-ffp-contract=off"] and "dw_stance_inverse.h" in build.HEADERS
    assert HEADER in open(os.path.join(ROOT, "isaacgymdyros_amd", "build.py")).read()          # (the staleness check's header list)
    K, KI = SM.K, IM.K
    assert K["DWK_ABI_VERSION"] == 1 and (K["DWK_NV"], K["DWK_MAX_CONTACTS"], K["DWK_ROWS"], K["DWK_MAX_ROWS"]) == (39, 4, 6, 24)
    assert all(K["DWK_" + k] == KI["DWI_" + k] for k in ("NUM_BODIES", "NUM_DOF", "NV", "MAX_CONTACTS", "ROWS", "MAX_ROWS", "GROUP", "LANES"))
    assert K["DWK_T_SOLE"] == KI["DWI_TABLE_WORDS"] and K["DWK_T_MU"] == K["DWK_T_SOLE"] + 4 * 5 and K["DWK_TABLE_WORDS"] == K["DWK_T_MU"] + 1 + 3
    assert K["DWK_TABLE_WORDS"] % 4 == 0 and (K["DWK_SOLE_WORDS"], K["DWK_MARGINS"]) == (5, 4)
    assert SM.DEFAULTS == {"contacts": IM.DEFAULTS["contacts"], "weights": None, "soles": "model", "friction": 1.0, "contact_accel": True, "margins": True,
                           "base_residual": True, "tau_full": False, "armature": True, "auto": False}
    from isaacgymdyros_amd import model_tensors as MT
    # the whole table of the model-tensor features, in cfg order: one table, no second one beside it
    assert MT.FEATURES == (("body_states", "BodyStates", ()), ("force_sensors", "ForceSensors", ("terrain",)), ("jacobians", "Jacobians", ()),
                           ("dynamics", "Dynamics", ()), ("forward_dynamics", "ForwardDynamics", ()), ("contact_dynamics", "ContactDynamics", ()),
                           ("contact_inverse_dynamics", "ContactInverseDynamics", ()), ("stance_inverse_dynamics", "StanceInverseDynamics", ("terrain",)))
    assert not hasattr(MT, "EXTENSIONS")
    # section 27's header is untouched
    assert KI["DWI_ABI_VERSION"] == 1 and sorted(IM.EXPORTS) == ["abi_version", "last_error", "pack_table", "solve"]


def test_table_words(host, api):
    """dwi_pack_table's 1168 words first, bit for bit (ones for the weights of a single contact included), then the soles and mu; the library
    and the g++ build pack the same table; the model's sole is the bounding rectangle of a foot's four sole corners."""
    iapi = cbind.declare(C.CDLL(build.build()), "dyros_contact_inverse_dynamics.h", "dwi_")
    model = load_model()
    assert SM.model_soles(model) == {6: [0.03, 0.0, -0.1585, 0.15, 0.085], 12: [0.03, 0.0, -0.1585, 0.15, 0.085]}
    for K in (1, 2, 4):
        cs = SR.SETS[K]
        ids, pos = CR.ids_of(cs), [p for _, p in cs]
        for w in WEIGHTS:
            so = SR.soles_of(cs)
            t = SM.pack_table(api, model, ids, pos, flat_weights(w, K), so, 0.8)
            assert t.dtype == U and t.shape == (SM.TABLE_WORDS,) and np.array_equal(t, host_table(host, cs, w, so, 0.8))
            assert np.array_equal(t[:IM.TABLE_WORDS], IM.pack_table(iapi, model, ids, pos, flat_weights(w, K)))
            if K == 1:
                assert np.array_equal(t[IM.K["DWI_T_W"]:IM.K["DWI_T_W"] + 6].view(F), np.ones(6, F))
            assert np.array_equal(t[SM.K["DWK_T_SOLE"]:SM.K["DWK_T_SOLE"] + 5 * K].view(F), so.reshape(-1)) and (t[SM.K["DWK_T_SOLE"] + 5 * K:SM.K["DWK_T_MU"]] == 0).all()
            assert t[SM.K["DWK_T_MU"]:SM.K["DWK_T_MU"] + 1].view(F)[0] == F(0.8) and (t[-3:] == 0).all()
        # no soles: points at the contacts' pos
        t = SM.pack_table(api, model, ids, pos)
        want = np.concatenate([np.asarray(pos, F), np.zeros((K, 2), F)], 1)
        assert np.array_equal(t[SM.K["DWK_T_SOLE"]:SM.K["DWK_T_SOLE"] + 5 * K].view(F), want.reshape(-1)) and t[SM.K["DWK_T_MU"]:SM.K["DWK_T_MU"] + 1].view(F)[0] == 1.0
    assert np.array_equal(SR.soles_of(SR.SETS[4]), np.asarray(SM.resolve({"contacts": [{"body": b, "pos": list(p)} for b, p in SR.SETS[4]]})["sole_words"], F))


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_pack_table_refusals(api):
    model = load_model()
    feet, pos = [8, 16], [[0, 0, -0.09]] * 2
    bad = ((([], []), "count must be in 1..DWC_MAX_CONTACTS"), (([1, 2, 3, 4, 5], [[0, 0, 0]] * 5), "count must be in 1..DWC_MAX_CONTACTS"),
           (([8, 38], pos), "a body id is outside 0..37"), (([-1], pos[:1]), "a body id is outside 0..37"),
           ((feet, [[0, 0, -0.09], [0, float("nan"), 0]]), "pos is not finite"), (([8, 6], pos), "two contacts on one moving body"),
           (([0, 0], pos), "two contacts on one moving body"))
    for (ids, p), msg in bad:
        with pytest.raises(cbind.DyrosWalkLibraryError, match="dwk_pack_table: " + msg):
            SM.pack_table(api, model, ids, p)
    for i, x in ((0, 0.0), (3, -1.0), (7, float("nan")), (11, float("inf")), (5, -0.0)):
        w = np.ones(12, F)
        w[i] = x
        with pytest.raises(cbind.DyrosWalkLibraryError, match=r"dwk_pack_table: a weight is not finite and positive \(index %d\)" % i):
            SM.pack_table(api, model, feet, pos, w)
    with pytest.raises(ValueError):
        SM.pack_table(api, model, feet, pos, np.ones(6, F))
    with pytest.raises(ValueError):
        SM.pack_table(api, model, feet, pos, None, np.zeros(5, F))
    good = np.array([SR.MODEL_SOLE] * 2, F)
    for (i, c), x, msg in (((0, 1), float("nan"), "a sole is not finite"), ((1, 4), float("inf"), "a sole is not finite"), ((1, 0), -float("inf"), "a sole is not finite"),
                           ((0, 3), -1e-6, "a half extent of a sole is negative"), ((1, 4), -1.0, "a half extent of a sole is negative")):
        so = good.copy()
        so[i, c] = x
        with pytest.raises(cbind.DyrosWalkLibraryError, match=r"dwk_pack_table: %s \(index %d\)" % (msg, i)):
            SM.pack_table(api, model, feet, pos, None, so)
    for mu in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(cbind.DyrosWalkLibraryError, match="dwk_pack_table: mu is not finite and positive"):
            SM.pack_table(api, model, feet, pos, None, good, mu)
    assert SM.pack_table(api, model, feet, pos, None, np.zeros((2, 5), F), 1e-3) is not None          # (a point, a small mu: accepted)
    d = {k: np.array(v) for k, v in model.d.items() if k in ("mv_parent", "mv_pos", "mv_rot0", "mv_axis", "body_moving", "inert_gym", "inert_mv", "inert_mass",
                                                             "inert_com", "inert_I")}
    d["mv_parent"][5] = 6
    with pytest.raises(cbind.DyrosWalkLibraryError, match="dwk_pack_table: a child precedes its parent"):
        SM.pack_table(api, d, feet, pos)
    t = np.zeros(SM.TABLE_WORDS, U)
    cst, mst = C.byref(CM.contacts_struct(feet, pos)), C.byref(JM.model_struct(model))
    for args in ((None, cst, None, None, 1.0, t.ctypes.data), (mst, None, None, None, 1.0, t.ctypes.data), (mst, cst, None, None, 1.0, None)):
        assert api["pack_table"](*args) == -1 and b"dwk_pack_table: a pointer is missing" in api["last_error"]()


def test_refusals_happen_before_any_launch(api):
    """Every buffer is NULL or a host address here: a launch would fault, a refusal returns -1 with its message."""
    one = C.c_void_p(16)
    ok = lambda **kw: tuple(dict(dict(n=8, table=one, root=one, dof=one, ms=None, arm=None, gx=0.0, gy=0.0, gz=-9.81, accel=None, fref=None, stance=None, vac=0,          # noqa: E731
                                      tau_joint=one, force=one, ca=None, tau_full=None, base=None, margins=None, feasible=None, stream=None), **kw).values())
    for args, msg in ((ok(n=0), b"num_envs"), (ok(n=-3), b"num_envs"), (ok(n=1 << 30), b"num_envs"),
                      (ok(table=None), b"a buffer is missing"), (ok(root=None), b"a buffer is missing"), (ok(dof=None), b"a buffer is missing"),
                      (ok(table=C.c_void_p(8)), b"16-byte aligned"), (ok(table=C.c_void_p(20)), b"16-byte aligned"),
                      (ok(tau_joint=None, force=None), b"no output"),
                      (ok(gx=float("nan")), b"gravity vector is not finite"), (ok(gz=float("inf")), b"gravity vector is not finite")):
        assert api["solve"](*args) == -1 and msg in api["last_error"]() and b"dwk_solve" in api["last_error"](), (args, api["last_error"]())


# ---------------------------------------------------------------------------------------------- 8. the kernel's resources
def test_kernel_uses_no_scratch_and_keeps_dwn_residency():
    """Exactly two kernels in the unit, dwi_k_solve and dwk_k_solve; dwk_k_solve: no scratch, LDS <= 40 960 B (four workgroups -- 16 envs --
    share a CU's 160 KB), occupancy no lower than dwn_k_inverse_dynamics's."""
    (_n, ri), (_nk, r), rn = RES.solve_kernels()
    assert r["scratch"] == 0
    print("dwk_k_solve: %d VGPRs, LDS %d bytes per workgroup (dwi %d), %d waves per SIMD (dwn %d)" % (r["vgprs"], r["lds"], ri["lds"], r["occ"], rn["occ"]))
    # dwi_k_solve's store, the table's 24 further words and a mask word per env
    assert r["lds"] <= ri["lds"] + 4 * (SM.TABLE_WORDS - IM.TABLE_WORDS + SM.GROUP) and r["lds"] <= 40960 and r["occ"] >= rn["occ"]


# ---------------------------------------------------------------------------------------------- 9. the Python surface
def test_cfg_spec():
    assert SM.resolve(None) is None and SM.resolve(False) is None
    full = SM.resolve(True)
    assert full == SM.resolve({}) and {k: full[k] for k in SM.DEFAULTS} == SM.DEFAULTS and full["ids"] == [8, 16] and full["pos"] == [[0.0, 0.0, -0.09]] * 2
    assert full["w"] is None and full["sole_words"] == [[0.03, 0.0, -0.1585, 0.15, 0.085]] * 2 and full["friction"] == 1.0
    sole = {"center": [0.0, 0.0, -0.1], "half": [0.1, 0.05]}
    s = SM.resolve({"contacts": [{"body": "base_link"}, {"body": 27, "pos": [0.1, 0, 0]}], "weights": [1, 1, 1, 10, 10, 10], "soles": [sole, None], "friction": 0.6,
                    "contact_accel": False, "margins": False, "base_residual": False, "tau_full": True, "auto": True, "armature": False})
    assert s["ids"] == [0, 27] and s["w"] == [1.0, 1.0, 1.0, 10.0, 10.0, 10.0] * 2 and s["friction"] == 0.6
    assert s["sole_words"] == [[0.0, 0.0, -0.1, 0.1, 0.05], [0.1, 0.0, 0.0, 0.0, 0.0]]
    assert SM.resolve({"contacts": [{"body": "base_link"}, {"body": "L_Foot_Link"}]})["sole_words"] == [[0.0] * 5, [0.03, 0.0, -0.1585, 0.15, 0.085]]
    foot = {"body": "L_Foot_Link"}
    for bad in (1, "on", ["weights"], {"h": True}, {"contact_accel": 1}, {"margins": 1}, {"base_residual": None}, {"tau_full": None}, {"armature": 1.0}, {"auto": "no"},
                {1: True}, {"weights": 1.0}, {"weights": [1] * 5}, {"weights": [1, 1, 1, 1, 1, 0]}, {"weights": [1, 1, 1, 1, 1, float("nan")]}, {"weights": [[1] * 6]},
                {"contacts": []}, {"contacts": [foot] * 5}, {"contacts": [{"body": "no_such_link"}]}, {"contacts": [foot, {"body": "L_AnkleRoll_Link"}]},
                {"friction": 0}, {"friction": -1.0}, {"friction": float("nan")}, {"friction": float("inf")}, {"friction": True}, {"friction": "1"}, {"friction": None},
                {"soles": "sole"}, {"soles": None}, {"soles": []}, {"soles": [sole]}, {"soles": [sole] * 3}, {"soles": [sole, {"center": [0, 0, 0]}]},
                {"soles": [sole, {"center": [0, 0], "half": [0.1, 0.1]}]}, {"soles": [sole, {"center": [0, 0, 0], "half": [0.1, -0.1]}]},
                {"soles": [sole, {"center": [0, 0, float("nan")], "half": [0.1, 0.1]}]}, {"soles": [sole, {"center": [0, 0, 0], "half": [0.1, float("inf")]}]},
                {"soles": [sole, {"center": [0, 0, 0], "half": [0.1, 0.1], "mu": 1}]}, {"soles": [sole, [0, 0, 0, 0.1, 0.1]]}, {"soles": {"center": [0, 0, 0], "half": [0, 0]}}):
        with pytest.raises(ValueError):
            SM.resolve(bad)
    # section 27's messages under the new name
    with pytest.raises(ValueError, match="stance_inverse_dynamics.contacts"):
        SM.resolve({"contacts": [{"body": "no_such_link"}]})
    with pytest.raises(ValueError, match="stance_inverse_dynamics.weights must be None, six finite positive numbers or 2 lists of six"):
        SM.resolve({"weights": [1] * 7})
    with pytest.raises(ValueError, match=r"stance_inverse_dynamics: unknown keys \['h'\]"):
        SM.resolve({"h": True})
    with pytest.raises(ValueError, match="stance_inverse_dynamics: plane only"):
        SM.resolve(True, terrain={"mesh_type": "heightfield"})
    from isaacgymdyros_amd.config import default_cfg, validate_cfg
    cfg = default_cfg(64, "cpu")
    assert "stance_inverse_dynamics" not in cfg["sim"]["mi355"] and "amp_stance_inverse_dynamics" not in cfg["sim"]["mi355"]          # (off by default)
    for key in ("stance_inverse_dynamics", "amp_stance_inverse_dynamics"):
        cfg = default_cfg(64, "cpu")
        cfg["sim"]["mi355"][key] = {"weights": [1, 1, 1, 10, 10, 10], "tau_full": True, "auto": True, "contacts": [foot], "soles": [sole], "friction": 0.5}
        validate_cfg(cfg)
        cfg["sim"]["mi355"][key] = True
        validate_cfg(cfg)
        for bad in ({"mass": True}, {"tau_full": 1}, {"weights": [1] * 7}, {"weights": [0] * 6}, "on", {"contacts": [foot, foot]}, {"friction": 0}, {"soles": [sole]}):
            cfg["sim"]["mi355"][key] = bad
            with pytest.raises(ValueError):
                validate_cfg(cfg)
        cfg["sim"]["mi355"][key] = True
        cfg["terrain"] = dict(cfg.get("terrain") or {}, mesh_type="heightfield")
        with pytest.raises(ValueError, match="plane only"):
            validate_cfg(cfg)
    # TocabiAMPLower keeps its own key from the physics host
    src = open(os.path.join(ROOT, "isaacgymdyros_amd", "tocabi_amp_lower.py")).read()
    assert re.search(r'k not in \([^)]*"amp_stance_inverse_dynamics"[^)]*\)', src)
