"""The contact inverse dynamics without a GPU (include/dyros_contact_inverse_dynamics.h, isaacgymdyros_amd/csrc/dw_contact_inverse.h, DESIGN.md
section 27): the reference (tests/contact_inverse_dynamics_ref.py) against things that are not itself -- the base rows, the round trip through
the dense KKT system of section 26, the chain's accelerations, optimality against null-space moves; the per-env arithmetic -- compiled by g++
from the headers the HIP kernel includes (tests/contact_inverse_dynamics_host.cpp) -- against the float64 reference under its measured
tolerance; the outputs' exact properties; the header, the Python binding and the built library; refusals; the kernel's resources; the cfg
surface."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import body_states_ref as R
import contact_dynamics_ref as CR
import contact_inverse_dynamics_ref as IR
import dynamics_ref as DR
import inverse_dynamics_resources as RES
from isaacgymdyros_amd import build, cbind
from isaacgymdyros_amd import contact_dynamics as CM
from isaacgymdyros_amd import contact_inverse_dynamics as IM
from isaacgymdyros_amd import jacobians as JM
from isaacgymdyros_amd.model import load_model
from test_body_states import TAKEN as TAKEN_BODIES          # noqa: F401
from test_gait_profile_abi import TAKEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dw_contact_inverse.hip"
N = 37
F = np.float32
U = np.uint32
OUTS = IR.OUTS
GRAV = DR.GRAVITY
WEIGHTS = (None, IR.MOMENTS_10)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------- 1. the reference against what is not itself
@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_reference_against_what_is_not_itself(K, vel_at_com):
    """At 64 seeded states, for unit weights and moments weighted 10 x, with a seeded f_ref, each within 1e-8 of the largest value (section
    26's bound): J_b' f = r[0:6]; (a, f) solves the dense KKT system of contact_dynamics_ref.evaluate's M, jc and jdnu for b = [0;
    tau_joint] - h and gamma = contact_accel (the system is assembled here in float64: evaluate() itself rounds its right-hand sides to
    float32); contact_accel = jc a + jdnu; and |f - f_ref|_W is no larger than for f + n, n seeded in the null space of J_b'."""
    cs, n, m = IR.SETS[K], 64, 6 * K
    root, dof, ms, arm, acc = DR.seeded(n, 3 + vel_at_com)
    fr = IR.fref_of(n, m, 5)
    kkt = CR.evaluate(root, dof, vel_at_com, ms, arm, cs)
    h = DR.evaluate(root, dof, vel_at_com, ms, arm)["bias"]
    a = acc.astype(np.float64)
    rng = np.random.default_rng(7)
    for w in WEIGHTS:
        o = IR.evaluate(root, dof, vel_at_com, ms, arm, cs, acc, w, fr)
        Jb = o["jc"][:, :, 0:6]
        base = np.abs(np.einsum("nrk,nr->nk", Jb, o["force"]) - o["tau_full"][:, 0:6]).max()
        assert base <= 1e-8 * np.abs(o["tau_full"][:, 0:6]).max()
        ca = np.abs(np.einsum("nrc,nc->nr", kkt["jc"], a) + kkt["jdnu"] - o["contact_accel"]).max()
        assert ca <= 1e-8 * np.abs(o["contact_accel"]).max()
        A = np.zeros((n, 39 + m, 39 + m))
        A[:, :39, :39], A[:, :39, 39:], A[:, 39:, :39] = kkt["M"], -np.swapaxes(kkt["jc"], 1, 2), kkt["jc"]
        right = np.concatenate([np.concatenate([np.zeros((n, 6)), o["tau_joint"]], 1) - h, o["contact_accel"] - kkt["jdnu"]], 1)
        sol = np.linalg.solve(A, right[..., None])[..., 0]
        ea, ef = np.abs(sol[:, :39] - a).max(), np.abs(sol[:, 39:] - o["force"]).max()
        print("K=%d vel_at_com=%d weights %s: base rows %.1e, contact_accel %.1e, round trip: accel %.1e of %.0f, force %.1e of %.0f"
              % (K, vel_at_com, w, base, ca, ea, np.abs(a).max(), ef, np.abs(o["force"]).max()))
        assert ea <= 1e-8 * np.abs(a).max() and ef <= 1e-8 * np.abs(o["force"]).max()
        if K == 1:
            continue
        # the null space of J_b' [6, m]: the last m - 6 right singular vectors
        null = np.linalg.svd(np.swapaxes(Jb, 1, 2))[2][:, 6:]          # [n, m - 6, m]
        move = np.einsum("nk,nkr->nr", rng.normal(0, 50.0, (n, m - 6)), null)
        assert np.abs(np.einsum("nrk,nr->nk", Jb, move)).max() <= 1e-8 * np.abs(move).max()
        cost = lambda f: np.sqrt((o["weights"] * (f - o["f_ref"]) ** 2).sum(-1))          # noqa: E731
        assert (cost(o["force"]) <= cost(o["force"] + move)).all() and (cost(o["force"]) <= cost(o["force"] + 1e-3 * move) + 1e-9).all()
    # with one contact neither the weights nor f_ref matter
    if K == 1:
        x, y = IR.evaluate(root, dof, vel_at_com, ms, arm, cs, acc), IR.evaluate(root, dof, vel_at_com, ms, arm, cs, acc, IR.MOMENTS_10, fr)
        assert np.abs(x["force"] - y["force"]).max() <= 1e-8 * np.abs(x["force"]).max()


def test_conditioning_of_g():
    """cond(G) over the STATES measured states: below 7 with unit weights, below 40 with moments weighted 10 x -- no pivoting is needed."""
    for v in (0, 1):
        for K in (1, 2, 4):
            unit, ten = IR.measured(v, K)["cond"], IR.measured(v, K, IR.MOMENTS_10)["cond"]
            print("vel_at_com=%d K=%d: cond(G) %.2f with unit weights, %.1f with moments weighted 10 x" % (v, K, unit, ten))
            assert unit < 7.0 and ten < 40.0


# ---------------------------------------------------------------------------------------------- 2. the g++ build against float64
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/contact_inverse_dynamics_host.cpp")
    d = tmp_path_factory.mktemp("dwih")
    so, so_n = str(d / "libdwih.so"), str(d / "libdwnh.so")
    for out, src in ((so, "contact_inverse_dynamics_host.cpp"), (so_n, "dynamics_host.cpp")):
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", out, os.path.join(ROOT, "tests", src)])
    lib = C.CDLL(so)
    lib.dwih_solve.argtypes = lib.dwih_solve_product.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_float] * 3 + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 4
    lib.dwih_pack_table.argtypes = [C.POINTER(JM.DwjModel), C.POINTER(CM.DwcContacts), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.model = JM.model_struct(load_model())
    lib.tables = {}
    lib.dyn = C.CDLL(so_n)
    lib.dyn.dwnh_inverse_dynamics.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_float] * 3 + [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    return lib


def flat_weights(weights, K):
    """[6 K] float32 as pack_table takes them, or None."""
    return None if weights is None else (np.tile(np.asarray(weights, F), K) if np.asarray(weights).size == 6 else np.asarray(weights, F).reshape(-1))


def host_table(lib, contacts, weights=None):
    key = (tuple(contacts), None if weights is None else tuple(np.asarray(weights, F).reshape(-1)))
    if key not in lib.tables:
        table, err = np.zeros(IM.TABLE_WORDS, U), C.create_string_buffer(256)
        st = CM.contacts_struct(CR.ids_of(contacts), [p for _, p in contacts])
        assert lib.dwih_pack_table(C.byref(lib.model), C.byref(st), _p(flat_weights(weights, len(contacts))), _p(table), err, 256) == 0, err.value
        lib.tables[key] = table
    return lib.tables[key]


def host_run(lib, contacts, root, dof, ms, arm, vel_at_com, accel=None, f_ref=None, weights=None, outs=OUTS, g=GRAV, expect=0, fn="dwih_solve"):
    """The outputs named, NaN-filled beforehand, as a dict (the others None).  fn: dwih_solve, section 27's plain row-ordered sums, stated in
    the host file only; or dwih_solve_product, the sums dwi_solve runs (contact by contact, every contact on)."""
    n, m = len(root), 6 * len(contacts)
    shape = {"tau_joint": (n, 33), "force": (n, m), "contact_accel": (n, m), "tau_full": (n, 39)}
    o = {k: np.full(shape[k], np.nan, F) if k in outs else None for k in OUTS}
    rc = getattr(lib, fn)(n, _p(host_table(lib, contacts, weights)), _p(root), _p(dof), _p(ms), _p(arm), g[0], g[1], g[2], _p(accel), _p(f_ref), vel_at_com,
                        *[_p(o[k]) for k in OUTS])
    assert rc == expect
    return o


def same(a, b):
    return np.array_equal(a.view(U), b.view(U))


def same_but_zero_signs(a, b):
    """The same bits, a zero's sign apart."""
    return bool(np.isfinite(a).all() and np.isfinite(b).all() and np.array_equal(a, b))


@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_host_build_against_float64(host, K, vel_at_com):
    """Every channel within 4 d of the float64 reference (force and tau_joint: d scaled with the solution), every word written: unit weights and
    moments weighted 10 x, with and without f_ref."""
    cs = IR.SETS[K]
    root, dof, ms, arm, acc = DR.seeded(N, 11 + vel_at_com)
    for w in WEIGHTS:
        for fr in (None, IR.fref_of(N, 6 * K, 13)):
            o = host_run(host, cs, root, dof, ms, arm, vel_at_com, acc, fr, w)
            assert all(np.isfinite(o[k]).all() for k in OUTS)
            want = IR.evaluate(root, dof, vel_at_com, ms, arm, cs, acc, w, fr)
            ex = IR.excess(o, want, vel_at_com, K, w, fr is not None,
                           report="host N=%d K=%d vel_at_com=%d weights %s f_ref %s" % (N, K, vel_at_com, "unit" if w is None else "10 x", fr is not None))
            assert len(ex) == len(IR.CHANNELS) and IR.within(ex), ex
    # K lists of six: another weight for every contact
    if K == 2:
        w = [[1.0, 1.0, 1.0, 10.0, 10.0, 10.0], [10.0, 10.0, 10.0, 10.0, 10.0, 10.0]]
        o = host_run(host, cs, root, dof, ms, arm, vel_at_com, acc, None, w)
        want = IR.evaluate(root, dof, vel_at_com, ms, arm, cs, acc, w)
        # (ratios of 1 and 10: under the d of moments weighted 10 x)
        ex = IR.excess(o, want, vel_at_com, K, IR.MOMENTS_10, False, report="host, the second foot ten times as dear")
        assert IR.within(ex), ex
        assert np.abs(want["force"][:, 6:9]).sum() < np.abs(want["force"][:, 0:3]).sum()          # (the dear foot carries less)


# ---------------------------------------------------------------------------------------------- 3. exact properties
def test_a_contact_on_the_base_returns_the_base_rows(host):
    """One contact on base_link at its origin, origin velocities: G is the identity exactly (the float32 restatement shows it), so force is
    tau_full[0:6] and tau_joint is tau_full[6:], bit for bit, a zero's sign apart."""
    root, dof, ms, arm, acc = DR.seeded(N, 21)
    o = host_run(host, IR.BASE, root, dof, ms, arm, 0, acc)
    assert same_but_zero_signs(o["force"], o["tau_full"][:, 0:6]) and same_but_zero_signs(o["tau_joint"], o["tau_full"][:, 6:])
    assert np.abs(o["tau_full"][:, 0:6]).min() > 0
    r = IR.restate(root, dof, 0, ms, arm, IR.BASE, acc)
    assert np.array_equal(r["G"], np.broadcast_to(np.eye(6, dtype=F), (N, 6, 6)))
    assert same_but_zero_signs(r["force"], r["tau_full"][:, 0:6]) and same_but_zero_signs(r["tau_joint"], r["tau_full"][:, 6:])


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_exact_properties(host, vel_at_com):
    v = vel_at_com
    root, dof, ms, arm, acc = DR.seeded(N, 23)
    zeros39 = np.zeros((N, 39), F)
    for K in (1, 2, 4):
        cs, m = IR.SETS[K], 6 * K
        fr = IR.fref_of(N, m, 25)
        o = host_run(host, cs, root, dof, ms, arm, v, acc, fr, IR.MOMENTS_10)
        assert all(np.isfinite(o[k]).all() for k in OUTS)
        # tau_full has the bits of the host build of dwn_inverse_dynamics for the same inputs; a NULL accel is dwn's tau for zeros, a zero's sign apart
        tau = np.full((N, 39), np.nan, F)
        table_n = np.ascontiguousarray(host_table(host, cs)[:IM.K["DWI_T_K"]])
        assert host.dyn.dwnh_inverse_dynamics(N, _p(table_n), _p(root), _p(dof), _p(ms), _p(arm), *GRAV, _p(acc), v, None, None, _p(tau), None) == 0
        assert same(tau, o["tau_full"])
        assert host.dyn.dwnh_inverse_dynamics(N, _p(table_n), _p(root), _p(dof), _p(ms), _p(arm), *GRAV, _p(zeros39), v, None, None, _p(tau), None) == 0
        on = host_run(host, cs, root, dof, ms, arm, v, None, fr, IR.MOMENTS_10)
        assert same_but_zero_signs(tau, on["tau_full"])
        # accel NULL equals zeros, f_ref NULL equals zeros
        oz = host_run(host, cs, root, dof, ms, arm, v, zeros39, fr, IR.MOMENTS_10)
        assert all(same_but_zero_signs(on[k], oz[k]) for k in OUTS) and not same(on["force"], o["force"])
        fn = host_run(host, cs, root, dof, ms, arm, v, acc, None, IR.MOMENTS_10)
        fz = host_run(host, cs, root, dof, ms, arm, v, acc, np.zeros((N, m), F), IR.MOMENTS_10)
        assert all(same(fn[k], fz[k]) for k in OUTS)
        # one contact: the same bits for any weights; two and more: the weights and f_ref enter
        plain = host_run(host, cs, root, dof, ms, arm, v, acc)
        assert all(same(plain[k], fn[k]) for k in OUTS) == (K == 1)
        assert same(plain["contact_accel"], o["contact_accel"]) and same(plain["tau_full"], o["tau_full"])
        # 640 m out: the same bits
        far = root.copy()
        far[:, 0:2] += np.array([640.0, -640.0], F)
        of = host_run(host, cs, far, dof, ms, arm, v, acc, fr, IR.MOMENTS_10)
        assert all(same(of[k], o[k]) for k in OUTS)
        # a NULL output leaves the others' bits
        for k in OUTS:
            one = host_run(host, cs, root, dof, ms, arm, v, acc, fr, IR.MOMENTS_10, outs=(k,))
            assert same(one[k], o[k]) and all(one[j] is None for j in OUTS if j != k), k
            rest = host_run(host, cs, root, dof, ms, arm, v, acc, fr, IR.MOMENTS_10, outs=tuple(j for j in OUTS if j != k))
            assert rest[k] is None and all(same(rest[j], o[j]) for j in OUTS if j != k), k
        # the base rows are carried: J_b' f = r[0:6] within what 4 d of force becomes through |J_b| and 4 d of dwn's tau
        want = IR.evaluate(root, dof, v, ms, arm, cs, acc, IR.MOMENTS_10, fr)
        Jb = want["jc"][:, :, 0:6]
        res = np.abs(np.einsum("nrk,nr->nk", Jb, o["force"].astype(np.float64)) - o["tau_full"][:, 0:6].astype(np.float64))
        dn = DR.measured(v)
        allow = (np.einsum("nrk,nr->nk", np.abs(Jb), IR.allowance(want, v, K, "force", IR.MOMENTS_10, True))
                 + IR.FACTOR * np.array([dn["tau_lin"]] * 3 + [dn["tau_ang"]] * 3))
        assert (res <= allow).all()


@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_product_sums_are_the_plain_row_ordered_sums(host, K, vel_at_com):
    """The sums dwi_solve runs -- contact by contact over the full mask, then a contact's six rows -- against section 27's plain statement, r =
    0 .. m - 1 with the contact r / 6: the same bits in all four outputs, moments weighted 10 x, with f_ref."""
    root, dof, ms, arm, acc = DR.seeded(N, 23)
    fr = IR.fref_of(N, 6 * K, 25)
    plain = host_run(host, IR.SETS[K], root, dof, ms, arm, vel_at_com, acc, fr, IR.MOMENTS_10)
    product = host_run(host, IR.SETS[K], root, dof, ms, arm, vel_at_com, acc, fr, IR.MOMENTS_10, fn="dwih_solve_product")
    assert all(np.isfinite(plain[k]).all() and same(product[k], plain[k]) for k in OUTS)


def test_non_finite_inputs_stay_in_their_env(host):
    cs = IR.SETS[2]
    root, dof, ms, arm, acc = DR.seeded(6, 41)
    fr = IR.fref_of(6, 12, 43)
    o0 = host_run(host, cs, root, dof, ms, arm, 1, acc, fr)
    root[2, 4], dof[3, 4, 0], acc[5, 7] = np.nan, np.inf, np.nan          # (DoF 4 drives moving body 5, on the left foot's path)
    o = host_run(host, cs, root, dof, ms, arm, 1, acc, fr)
    for k in OUTS:
        assert same(o[k][[0, 1, 4]], o0[k][[0, 1, 4]]), k
        assert np.isnan(o[k][2]).any() and np.isnan(o[k][3]).any(), k
    assert all(np.isnan(o[k][5]).any() for k in ("tau_joint", "force", "tau_full"))


@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_at_rest_the_contacts_carry_the_weight(host, K, vel_at_com):
    """nu = 0 and a = 0: the contacts' forces sum to dwn's gravity[0:3], within the sum of the forces' allowances and 4 d of gravity's."""
    root, dof, ms, arm, _acc = DR.seeded(N, 51)
    root[:, 7:13] = 0
    dof = dof.reshape(N, 33, 2).copy()
    dof[:, :, 1] = 0
    dof = np.ascontiguousarray(dof.reshape(N, -1))
    o = host_run(host, IR.SETS[K], root, dof, ms, arm, vel_at_com)
    want = IR.evaluate(root, dof, vel_at_com, ms, arm, IR.SETS[K])
    grav = DR.evaluate(root, dof, vel_at_com, ms, arm)["gravity"][:, 0:3]
    total = o["force"].astype(np.float64).reshape(N, K, 6)[:, :, 0:3].sum(1)
    allow = IR.allowance(want, vel_at_com, K, "force").reshape(N, K, 6)[:, :, 0:3].sum(1) + IR.FACTOR * DR.measured(vel_at_com)["gravity_lin"]
    print("K=%d: the forces' sum against gravity[0:3] (up to %.0f N): %.3f of the allowance" % (K, np.abs(grav).max(), (np.abs(total - grav) / allow).max()))
    assert (np.abs(total - grav) <= allow).all() and grav[:, 2].min() > 500.0


# ---------------------------------------------------------------------------------------------- 4. the ABI
@pytest.fixture(scope="module")
def api():
    return cbind.declare(C.CDLL(build.build()), "dyros_contact_inverse_dynamics.h", "dwi_")


@pytest.mark.parametrize("check", ["prototypes", "layouts"])
def test_header_python_and_library_agree(check, tmp_path):
    import test_cbind as TC
    if check == "prototypes":
        TC.test_ctypes_prototypes_match_the_header("dyros_contact_inverse_dynamics.h", "dwi_", "contact_inverse_dynamics", C.CDLL(build.build()))
    else:
        TC.test_struct_layouts_match_the_host_compiler("dyros_contact_inverse_dynamics.h", "dwi_", "contact_inverse_dynamics", tmp_path)
    assert sorted(IM.EXPORTS) == ["abi_version", "last_error", "pack_table", "solve"]
    assert dict(build.SOURCES)[SRC] == ["-ffp-contract=off"] and "dw_contact_inverse.h" in build.HEADERS
    K, KC, KN = IM.K, CM.K, cbind.constants("dyros_dynamics.h", "dwn_")
    assert K["DWI_ABI_VERSION"] == 1 and (K["DWI_NV"], K["DWI_MAX_CONTACTS"], K["DWI_ROWS"], K["DWI_MAX_ROWS"]) == (39, 4, 6, 24)
    assert (K["DWI_NUM_BODIES"], K["DWI_NUM_DOF"], K["DWI_MAX_CONTACTS"]) == (KC["DWC_NUM_BODIES"], KC["DWC_NUM_DOF"], KC["DWC_MAX_CONTACTS"])
    assert (K["DWI_GROUP"], K["DWI_LANES"]) == (KN["DWN_GROUP"], KN["DWN_LANES"])
    assert K["DWI_T_K"] == KN["DWN_TABLE_WORDS"] and K["DWI_T_CONTACT"] == K["DWI_T_K"] + 1 and K["DWI_T_W"] == K["DWI_T_CONTACT"] + 16
    assert K["DWI_TABLE_WORDS"] == K["DWI_T_W"] + 24 + 3 and K["DWI_TABLE_WORDS"] % 4 == 0
    assert IM.DEFAULTS == {"contacts": [{"body": "L_Foot_Link", "pos": [0.0, 0.0, -0.09]}, {"body": "R_Foot_Link", "pos": [0.0, 0.0, -0.09]}], "weights": None,
                           "contact_accel": True, "tau_full": False, "armature": True, "auto": False}
    # (model_tensors.FEATURES is pinned whole, this feature's row included, in tests/test_stance_inverse_dynamics.py)
    # the older headers are untouched
    assert KC["DWC_ABI_VERSION"] == 1 and KN["DWN_ABI_VERSION"] == 1 and JM.K["DWJ_ABI_VERSION"] == 1


def test_the_library_and_the_host_build_pack_the_same_table(host, api):
    napi = cbind.declare(C.CDLL(build.build()), "dyros_dynamics.h", "dwn_")
    capi = cbind.declare(C.CDLL(build.build()), "dyros_contact_dynamics.h", "dwc_")
    model = load_model()
    from isaacgymdyros_amd import dynamics as DM
    for K in (1, 2, 4):
        cs = IR.SETS[K]
        ids, pos = CR.ids_of(cs), [p for _, p in cs]
        for w in WEIGHTS:
            t = IM.pack_table(api, model, ids, pos, flat_weights(w, K))
            assert t.dtype == U and t.shape == (IM.TABLE_WORDS,) and np.array_equal(t, host_table(host, cs, w))
            assert np.array_equal(t[:IM.K["DWI_T_K"]], DM.pack_table(napi, model)) and t[IM.K["DWI_T_K"]] == K
            c = CM.pack_table(capi, model, ids, pos)
            assert np.array_equal(t[IM.K["DWI_T_CONTACT"]:IM.K["DWI_T_W"]], c[CM.K["DWC_T_CONTACT"]:CM.K["DWC_T_CONTACT"] + 16])
            wt = t[IM.K["DWI_T_W"]:IM.K["DWI_T_W"] + 24].view(F)
            want = np.ones(6 * K, F) if w is None or K == 1 else flat_weights(w, K)          # (one contact: ones, f does not depend on W)
            assert np.array_equal(wt[:6 * K], want) and (wt[6 * K:].view(U) == 0).all() and (t[-3:] == 0).all()


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_pack_table_refusals(api):
    model = load_model()
    feet, pos = [8, 16], [[0, 0, -0.09]] * 2
    bad = ((([], []), "count must be in 1..DWC_MAX_CONTACTS"), (([1, 2, 3, 4, 5], [[0, 0, 0]] * 5), "count must be in 1..DWC_MAX_CONTACTS"),
           (([8, 38], pos), "a body id is outside 0..37"), (([-1], pos[:1]), "a body id is outside 0..37"),
           ((feet, [[0, 0, -0.09], [0, float("nan"), 0]]), "pos is not finite"), (([8, 6], pos), "two contacts on one moving body"),
           (([0, 0], pos), "two contacts on one moving body"))
    for (ids, p), msg in bad:
        with pytest.raises(cbind.DyrosWalkLibraryError, match="dwi_pack_table: " + msg):
            IM.pack_table(api, model, ids, p)
    for i, x in ((0, 0.0), (3, -1.0), (7, float("nan")), (11, float("inf")), (5, -0.0)):
        w = np.ones(12, F)
        w[i] = x
        with pytest.raises(cbind.DyrosWalkLibraryError, match=r"dwi_pack_table: a weight is not finite and positive \(index %d\)" % i):
            IM.pack_table(api, model, feet, pos, w)
    w = np.ones(6, F)
    w[2] = 0.0
    with pytest.raises(cbind.DyrosWalkLibraryError, match="dwi_pack_table: a weight is not finite and positive"):          # (checked for one contact too)
        IM.pack_table(api, model, feet[:1], pos[:1], w)
    with pytest.raises(ValueError):
        IM.pack_table(api, model, feet, pos, np.ones(6, F))          # (six weights for two contacts: 12 are read)
    # it refuses what dwn_pack_table refuses, under its own name
    d = {k: np.array(v) for k, v in model.d.items() if k in ("mv_parent", "mv_pos", "mv_rot0", "mv_axis", "body_moving", "inert_gym", "inert_mv", "inert_mass",
                                                             "inert_com", "inert_I")}
    d["mv_parent"][5] = 6
    with pytest.raises(cbind.DyrosWalkLibraryError, match="dwi_pack_table: a child precedes its parent"):
        IM.pack_table(api, d, feet, pos)
    d["mv_parent"][5] = model.d["mv_parent"][5]
    d["inert_I"][9][1][1] = float("nan")
    with pytest.raises(cbind.DyrosWalkLibraryError, match="dwi_pack_table: inert_I is not finite"):
        IM.pack_table(api, d, feet, pos)
    t = np.zeros(IM.TABLE_WORDS, U)
    assert api["pack_table"](None, C.byref(CM.contacts_struct(feet, pos)), None, t.ctypes.data) == -1 and b"a pointer is missing" in api["last_error"]()
    assert api["pack_table"](C.byref(JM.model_struct(model)), None, None, t.ctypes.data) == -1 and b"a pointer is missing" in api["last_error"]()
    assert api["pack_table"](C.byref(JM.model_struct(model)), C.byref(CM.contacts_struct(feet, pos)), None, None) == -1 and b"a pointer is missing" in api["last_error"]()


def test_refusals_happen_before_any_launch(api):
    """Every buffer is NULL or a host address here: a launch would fault, a refusal returns -1 with its message."""
    one = C.c_void_p(16)
    ok = lambda **kw: tuple(dict(dict(n=8, table=one, root=one, dof=one, ms=None, arm=None, gx=0.0, gy=0.0, gz=-9.81, accel=None, fref=None, vac=0,          # noqa: E731
                                      tau_joint=one, force=one, ca=None, tau_full=None, stream=None), **kw).values())
    for args, msg in ((ok(n=0), b"num_envs"), (ok(n=-3), b"num_envs"), (ok(n=1 << 30), b"num_envs"),
                      (ok(table=None), b"a buffer is missing"), (ok(root=None), b"a buffer is missing"), (ok(dof=None), b"a buffer is missing"),
                      (ok(table=C.c_void_p(8)), b"16-byte aligned"), (ok(table=C.c_void_p(20)), b"16-byte aligned"),
                      (ok(tau_joint=None, force=None), b"no output"),
                      (ok(gx=float("nan")), b"gravity vector is not finite"), (ok(gz=float("inf")), b"gravity vector is not finite")):
        assert api["solve"](*args) == -1 and msg in api["last_error"]() and b"dwi_solve" in api["last_error"](), (args, api["last_error"]())


# ---------------------------------------------------------------------------------------------- 6. the kernel's resources
def test_kernel_uses_no_scratch_and_keeps_dwn_residency():
    """Exactly two kernels in the unit, dwi_k_solve and dwk_k_solve; dwi_k_solve: no scratch; its LDS is no more than
    dwn_k_inverse_dynamics's group plus the tail (the table's 44 further words, and per env the points 12, G 6 x 7, y 6, f 24 and f_ref 24 =
    108 words), and four workgroups -- 16 envs -- still share a CU's 160 KB."""
    (n, r), _dwk, rn = RES.solve_kernels()
    assert r["scratch"] == 0
    tail = 4 * ((IM.K["DWI_TABLE_WORDS"] - IM.K["DWI_T_K"]) + IM.GROUP * (12 + 6 * 7 + 6 + 24 + 24))
    print("dwi_k_solve: %d VGPRs, LDS %d bytes per workgroup (dwn %d, the tail %d), %d waves per SIMD (dwn %d)" % (r["vgprs"], r["lds"], rn["lds"], tail, r["occ"], rn["occ"]))
    assert r["lds"] <= rn["lds"] + tail and r["lds"] <= 160 * 1024 // 4 and r["occ"] >= rn["occ"]
    assert not any(x in n for x in tuple(TAKEN) + tuple(TAKEN_BODIES) + ("dwg_k_", "dwb_k_", "dwf_k_", "dwj_k_", "dwn_k_", "dwl_k_", "dwc_k_")), n
    assert not any(x in n for x in ("k_mlp", "k_wgrad", "k_policy", "k_adam", "k_grad_stats", "k_finish", "k_gae", "k_roll_pre", "k_roll_post", "k_loss",
                                    "k_relu_bwd", "k_bias_relu", "k_stage_obs", "k_retile", "dw_k_amp", "dw_k_newwalk", "dw_k_body_positions")), n


# ---------------------------------------------------------------------------------------------- 7. the Python surface
def test_cfg_spec():
    assert IM.resolve(None) is None and IM.resolve(False) is None
    full = IM.resolve(True)
    assert full == IM.resolve({}) and {k: full[k] for k in IM.DEFAULTS} == IM.DEFAULTS and full["ids"] == [8, 16] and full["pos"] == [[0.0, 0.0, -0.09]] * 2
    assert full["w"] is None
    s = IM.resolve({"contacts": [{"body": "base_link"}, {"body": 27, "pos": [0.1, 0, 0]}], "weights": [1, 1, 1, 10, 10, 10], "contact_accel": False, "tau_full": True,
                    "auto": True, "armature": False})
    assert s["ids"] == [0, 27] and s["pos"] == [[0.0, 0.0, 0.0], [0.1, 0.0, 0.0]] and s["w"] == [1.0, 1.0, 1.0, 10.0, 10.0, 10.0] * 2
    assert s["tau_full"] and s["auto"] and not (s["contact_accel"] or s["armature"])
    assert IM.resolve({"weights": [[1] * 6, [2.5] * 6]})["w"] == [1.0] * 6 + [2.5] * 6
    foot = {"body": "L_Foot_Link"}
    assert IM.resolve({"contacts": [foot], "weights": [[3.0] * 6]})["w"] == [3.0] * 6
    for bad in (1, "on", ["weights"], {"h": True}, {"rhs": 1}, {"contact_accel": 1}, {"tau_full": None}, {"armature": 1.0}, {"auto": "no"}, {1: True},
                {"weights": 1.0}, {"weights": []}, {"weights": [1] * 5}, {"weights": [1] * 12}, {"weights": [1, 1, 1, 1, 1, 0]}, {"weights": [1, 1, 1, 1, 1, -2.0]},
                {"weights": [1, 1, 1, 1, 1, float("nan")]}, {"weights": [1, 1, 1, 1, 1, float("inf")]}, {"weights": [1, 1, 1, 1, 1, True]}, {"weights": "111111"},
                {"weights": [[1] * 6]}, {"weights": [[1] * 6] * 3}, {"weights": [[1] * 6, [1] * 5]}, {"weights": [[1] * 6, [1, 1, 1, 1, 1, "x"]]},
                {"contacts": [foot], "weights": [[1] * 6] * 2},
                {"contacts": []}, {"contacts": "L_Foot_Link"}, {"contacts": [foot] * 5}, {"contacts": [{"pos": [0, 0, 0]}]}, {"contacts": [{"body": "no_such_link"}]},
                {"contacts": [{"body": 38}]}, {"contacts": [{"body": 8, "pos": [0, 0]}]}, {"contacts": [foot, {"body": "L_AnkleRoll_Link"}]}, {"contacts": [foot, {"body": 7}]}):
        with pytest.raises(ValueError):
            IM.resolve(bad)
    with pytest.raises(ValueError, match="contact_inverse_dynamics.contacts"):
        IM.resolve({"contacts": [{"body": "no_such_link"}]})
    from isaacgymdyros_amd.config import default_cfg, validate_cfg
    cfg = default_cfg(64, "cpu")
    assert "contact_inverse_dynamics" not in cfg["sim"]["mi355"] and "amp_contact_inverse_dynamics" not in cfg["sim"]["mi355"]          # (off by default)
    for key in ("contact_inverse_dynamics", "amp_contact_inverse_dynamics"):
        cfg = default_cfg(64, "cpu")
        cfg["sim"]["mi355"][key] = {"weights": [1, 1, 1, 10, 10, 10], "tau_full": True, "auto": True, "contacts": [foot]}
        validate_cfg(cfg)
        cfg["sim"]["mi355"][key] = True
        validate_cfg(cfg)
        for bad in ({"mass": True}, {"tau_full": 1}, {"weights": [1] * 7}, {"weights": [0] * 6}, "on", {"contacts": [foot, foot]}):
            cfg["sim"]["mi355"][key] = bad
            with pytest.raises(ValueError):
                validate_cfg(cfg)
    # TocabiAMPLower keeps its own key from the physics host
    src = open(os.path.join(ROOT, "isaacgymdyros_amd", "tocabi_amp_lower.py")).read()
    assert re.search(r'k not in \([^)]*"amp_contact_inverse_dynamics"[^)]*\)', src)
