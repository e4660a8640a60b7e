"""The inverse kinematics without a GPU (include/dyros_inverse_kinematics.h, isaacgymdyros_amd/csrc/dw_inverse_kinematics.h, DESIGN.md section
29): the reference (tests/inverse_kinematics_ref.py) against things that are not itself; the per-env arithmetic -- compiled by g++ from the
headers the HIP kernel includes (tests/inverse_kinematics_host.cpp) -- against the float64 reference under its measured tolerance, one step
and to convergence; the outputs' exact properties; injected faults; the header, the Python binding and the built library; refusals; the
kernel's resources; the cfg surface."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import body_states_ref as R
import contact_dynamics_ref as CR
import inverse_dynamics_resources as RES
import inverse_kinematics_ref as QR
from isaacgymdyros_amd import build, cbind
from isaacgymdyros_amd import contact_dynamics as CM
from isaacgymdyros_amd import inverse_kinematics as QM
from isaacgymdyros_amd import jacobians as JM
from isaacgymdyros_amd.model import load_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dw_inverse_kinematics.hip"
HEADER = "dyros_inverse_kinematics.h"
N = 37
F = np.float32
U = np.uint32
OUTS = QR.OUTS
WEIGHTS = (None, QR.ORI_10)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def params_of(P) -> QM.DwqParams:
    return QM.params_struct({"iterations": P["iterations"], "damping": float(P["damping"]), "max_step": float(P["max_step"]), "tol_pos": float(P["tol_pos"]),
                             "tol_ang": float(P["tol_ang"]), "base": P["base"], "limits": P["limits"], "target_frame": "root" if P["rel_root"] else "world"})


def table_args(P):
    """What a pack_table takes after the model, from a reference problem: the targets, the masks, the weights, the limits, the params."""
    cs = P["contacts"]
    return (CM.contacts_struct(CR.ids_of(cs), [p for _, p in cs]), np.ascontiguousarray(P["rows"], np.uint8), np.ascontiguousarray(P["w"], F),
            np.ascontiguousarray(P["dofs"], np.uint8), QR.LOWER, QR.UPPER, params_of(P))


def shapes(n, m):
    return {"q": ((n, 33), F), "root": ((n, 7), F), "residual": ((n, m), F), "err": ((n, 2), F), "iters": ((n,), np.int32), "converged": ((n,), np.uint8)}


def dof_of(q):
    """dof_state rows [n, 33, 2] with seeded rates, which the solve never reads."""
    d = np.random.default_rng(9).uniform(-4, 4, (len(q), 33, 2)).astype(F)
    d[:, :, 0] = q
    return d


# ---------------------------------------------------------------------------------------------- 1. the reference against what is not itself
@pytest.mark.parametrize("base", [False, True])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_reference_against_what_is_not_itself(K, base):
    """In float64 at 64 seeded cases: the lstsq step is J' (J J' + lambda^2 W^-1)^-1 e by np.linalg.solve within 1e-9; it is the minimiser of
    |W^1/2 (J dnu - e)|^2 + lambda^2 |dnu|^2 (no seeded move lowers the cost); finite differences of the error rows about a met target give -J; and where the
    loop converges, the float64 chain at the returned (base, q) puts the points within the tolerances of the targets."""
    P = QR.problem(K, base=base, weights=QR.ORI_10, rows=QR.MIXED[K], damping=0.05)
    root, q0, tgt, _ = QR.case(64, 3, P)
    c, pt, qb = QR.forward(root, q0, P)
    e, dead = QR.errors(c, pt, qb, tgt, P)
    J = QR.jac_of(c, P)
    assert not dead.any()
    dv = QR.dnu_lstsq(J, e, P)
    A = QR.a_of(J, P)
    want = np.einsum("nrc,nr->nc", J, np.linalg.solve(A, e[..., None])[..., 0])
    assert np.abs(dv - want).max() <= 1e-9 * np.abs(want).max()
    w, lam = P["w"].astype(np.float64), float(P["damping"])
    cost = lambda x: (w * (np.einsum("nrc,nc->nr", J, x) - e) ** 2).sum(-1) + lam * lam * (x * x).sum(-1)          # noqa: E731
    move = np.random.default_rng(5).normal(0, 1e-3, dv.shape)
    assert (cost(dv) <= cost(dv + move)).all()
    # -de/dnu = J along every free column, by central differences of 1e-6, where the error is zero (2 sign(w) v is the rotation vector to
    # first order only)
    cols, at = np.flatnonzero(QR.cols_of(P)), QR.targets_of(root, q0, P)
    for col in cols[:: max(1, len(cols) // 6)]:
        h = np.zeros((64, 39))
        h[:, col] = 1e-6
        es = []
        for s in (1.0, -1.0):
            r = QR.base_update(root.astype(np.float64), s * h)
            cc, pp, qq = QR.forward(r, q0.astype(np.float64) + s * h[:, 6:], P)
            es.append(QR.errors(cc, pp, qq, at, P)[0])
        assert np.abs((es[1] - es[0]) / 2e-6 - J[:, :, col]).max() <= 1e-6 * max(1.0, np.abs(J[:, :, col]).max())
    out = QR.solve(root, q0, tgt, dict(P, iterations=64, damping=0.01))
    ok = out["converged"] == 1
    assert ok.sum() >= 48
    res = QR.residual64(out, root, tgt, P).reshape(64, K, 6)[ok]
    assert np.abs(res[..., 0:3]).max() <= 1e-5 and np.abs(res[..., 3:6]).max() <= 1e-5


def test_conditioning_of_a():
    """cond(A) over the STATES seeded states, unit weights, a fixed base: at the smallest damping dwq_pack_table takes it stays inside the 8.0e5
    that section 26 factors without pivoting; a quarter less damping would not."""
    rows = {lam: (QR.cond_of(2, lam), QR.cond_of(4, lam)) for lam in (0.003, QM.MIN_DAMPING, 0.05)}
    for lam, (two, four) in rows.items():
        print("lambda %g: cond(A) at most %.3g (both feet), %.3g (four targets); free base %.3g, %.3g" % (lam, two, four, QR.cond_of(2, lam, True), QR.cond_of(4, lam, True)))
    assert QM.MIN_DAMPING == 4e-3 and max(rows[QM.MIN_DAMPING]) < 8.0e5 < rows[0.003][1]
    assert max(rows[0.05]) < 5e3 and QR.cond_of(4, QM.MIN_DAMPING, True) < QR.cond_of(4, QM.MIN_DAMPING)


# ---------------------------------------------------------------------------------------------- 2. the g++ build against float64
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/inverse_kinematics_host.cpp")
    so = str(tmp_path_factory.mktemp("dwqh") / "libdwqh.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, os.path.join(ROOT, "tests", "inverse_kinematics_host.cpp")])
    lib = C.CDLL(so)
    lib.dwqh_solve.argtypes = [C.c_int] + [C.c_void_p] * 11
    lib.dwqh_pack_table.argtypes = [C.POINTER(JM.DwjModel), C.POINTER(CM.DwcContacts)] + [C.c_void_p] * 5 + [C.POINTER(QM.DwqParams), C.c_void_p, C.c_char_p, C.c_int]
    lib.model = JM.model_struct(load_model())
    return lib


def host_table(lib, P):
    table, err = np.zeros(QM.TABLE_WORDS, U), C.create_string_buffer(256)
    st, rm, w, dm, lo, hi, pr = table_args(P)
    assert lib.dwqh_pack_table(C.byref(lib.model), C.byref(st), _p(rm), _p(w), _p(dm), _p(lo), _p(hi), C.byref(pr), _p(table), err, 256) == 0, err.value
    return table


def host_run(lib, P, root, q0, tgt, outs=OUTS, dof=None, pass_q0=False):
    """The outputs named, NaN-filled (integers: -1, 9) beforehand, as a dict (the others None).  dof: the dof_state rows (None: q0 and seeded
    rates); pass_q0: hand q0 over as the q0 argument, over rows whose positions are something else."""
    n = len(root)
    o = {k: (np.full(s, np.nan, t) if t == F else np.full(s, -1 if t == np.int32 else 9, t)) if k in outs else None for k, (s, t) in shapes(n, P["m"]).items()}
    rows = dof_of(q0 if not pass_q0 else q0[::-1] + F(0.1)) if dof is None else dof
    rc = lib.dwqh_solve(n, _p(host_table(lib, P)), _p(np.ascontiguousarray(root)), _p(rows), _p(np.ascontiguousarray(q0)) if pass_q0 else None,
                        _p(np.ascontiguousarray(tgt)), *[_p(o[k]) for k in OUTS])
    assert rc == 0
    return o


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("base", [False, True])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_one_step_against_float64(host, K, base):
    """iterations = 1: q, the residual rows (as returned and recomputed in float64 from the returned q) and the base pose within 4 d of the
    float64 lstsq step, every word written: unit weights and orientation rows weighted 10 x, with and without a row mask."""
    for w in WEIGHTS:
        for rows in (None, QR.MIXED[K]):
            P = QR.problem(K, rows=rows, weights=w, base=base, iterations=1)
            root, q0, tgt, _ = QR.case(N, 11, P)
            o = host_run(host, P, root, q0, tgt)
            assert all(np.isfinite(o[k]).all() for k in OUTS) and (o["iters"] == 1).all() and (o["converged"] == 0).all()
            want = QR.step(root, q0, tgt, P)
            ex = QR.excess(o, want, root, tgt, P, report="host one step K=%d base=%d weights %s rows %s" % (K, base, "unit" if w is None else "10 x", rows))
            assert len(ex) == len(QR.CHANNELS) and QR.within(ex), ex
            assert same(o["err"], np.stack([np.abs(o["residual"].reshape(N, K, 6)[..., 0:3]).max((1, 2)), np.abs(o["residual"].reshape(N, K, 6)[..., 3:6]).max((1, 2))], -1))
            # the update is no small thing: the step moves the joints by three orders of magnitude more than the allowance
            assert np.abs(want["q"] - q0).max() > 1e3 * QR.FACTOR * QR.measured(P)["q"]


@pytest.mark.parametrize("base", [False, True])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_convergence(host, K, base):
    """Reachable targets, at most 8 updates: the float64 reference converges on every case (checked first: no case is left out); the float32
    build reports converged on every case; its residual, recomputed in float64 from the returned q, is within 4 d of the reference's and within
    the tolerances plus that; with both feet on a fixed base -- square, locally unique -- q is within 4 d of the float64 solution."""
    P, root, q0, tgt, want = QR.conv_case(K, base)
    assert (want["converged"] == 1).all() and want["iters"].max() <= P["iterations"] and want["iters"].min() >= 2
    o = host_run(host, P, root, q0, tgt)
    assert (o["converged"] == 1).all() and (o["iters"] >= 2).all() and (o["iters"] <= P["iterations"]).all()
    assert (o["err"][:, 0] <= P["tol_pos"]).all() and (o["err"][:, 1] <= P["tol_ang"]).all()
    keep = ("rq_pos", "rq_ang") + (("q",) if K == 2 and not base else ())
    ex = {k: v for k, v in QR.excess(o, want, root, tgt, P, report="host convergence K=%d base=%d" % (K, base)).items() if k in keep}
    assert len(ex) == len(keep) and QR.within(ex), ex
    d = QR.measured(P)
    res = QR.residual64(o, root, tgt, P).reshape(len(root), K, 6)
    assert np.abs(res[..., 0:3]).max() <= P["tol_pos"] + QR.FACTOR * d["rq_pos"] and np.abs(res[..., 3:6]).max() <= P["tol_ang"] + QR.FACTOR * d["rq_ang"]


# ---------------------------------------------------------------------------------------------- 3. exact properties
@pytest.mark.parametrize("base", [False, True])
def test_exact_properties(host, base):
    for K in (1, 2, 4):
        P = QR.problem(K, base=base, iterations=6)
        root, q0, tgt, _ = QR.case(N, 23, P)
        o = host_run(host, P, root, q0, tgt)
        assert all(np.isfinite(o[k]).all() for k in OUTS)
        # unmasked joints return q0's bits; a fixed base returns the root's bits
        assert same(o["q"][:, ~P["dofs"]], q0[:, ~P["dofs"]]) and not (o["q"][:, P["dofs"]] == q0[:, P["dofs"]]).all(0).any()
        assert same(o["root"], np.ascontiguousarray(root[:, 0:7])) == (not base)
        # a NULL q0 and q0 = dof_state's positions: the same bits; so is q0 handed over rows that hold other positions
        viaq0 = host_run(host, P, root, q0, tgt, pass_q0=True)
        both = host_run(host, P, root, q0, tgt, dof=dof_of(q0), pass_q0=True)
        assert all(same(viaq0[k], o[k]) and same(both[k], o[k]) for k in OUTS)
        # a NULL output leaves the others' bits
        for k in OUTS:
            one = host_run(host, P, root, q0, tgt, outs=(k,))
            assert same(one[k], o[k]) and all(one[j] is None for j in OUTS if j != k), k
        # targets in the root's frame: an env moved 640 m gets the same bits
        Pr = dict(P, rel_root=True)
        rel = tgt.copy()
        rel[..., 0:3] -= root[:, None, 0:3]
        far = root.copy()
        far[:, 0:2] += np.array([640.0, -640.0], F)
        a, b = host_run(host, Pr, root, q0, rel), host_run(host, Pr, far, q0, rel)
        assert all(same(a[k], b[k]) for k in OUTS if k != "root") and same(a["root"][:, 3:7], b["root"][:, 3:7]) and same(a["root"][:, 2], b["root"][:, 2])
        if not base:
            assert same(b["root"], np.ascontiguousarray(far[:, 0:7]))
        # in the world frame the error's first difference is formed first, so 640 m out costs the targets' rounding alone: half an ulp of 640
        # (3.1e-5) on each of the m position words, to which one update answers with at most |de| / (2 lambda); six updates
        tf = tgt.copy()
        tf[..., 0:2] += np.array([640.0, -640.0], F)
        w = host_run(host, P, far, q0, tf)
        assert np.abs(w["q"] - o["q"]).max() <= 6 * np.sqrt(P["m"]) * 3.1e-5 / (2 * 0.05)


@pytest.mark.parametrize("K", [1, 2, 4])
def test_targets_from_the_state_take_no_update(host, K):
    """Targets that are the bodies' poses at q0 (the float64 chain's, rounded): iters 0, converged 1, q = q0 and the root bit for bit; a
    position-only target leaves its orientation rows +0.0 whatever the target's orientation."""
    for base in (False, True):
        P = QR.problem(K, base=base)
        root, q0, _tgt, _ = QR.case(N, 29, P)
        o = host_run(host, P, root, q0, QR.targets_of(root, q0, P))
        assert (o["iters"] == 0).all() and (o["converged"] == 1).all() and same(o["q"], q0) and same(o["root"], np.ascontiguousarray(root[:, 0:7]))
        assert (o["err"] <= 1e-5).all()
    P = QR.problem(K, rows=("position",) * K, iterations=4)
    root, q0, tgt, _ = QR.case(N, 31, P)
    spun = tgt.copy()
    spun[..., 3:7] = R.states(N * K, 33)[0][:, 3:7].reshape(N, K, 4)
    a, b = host_run(host, P, root, q0, tgt), host_run(host, P, root, q0, spun)
    assert all(same(a[k], b[k]) for k in OUTS)
    assert (a["residual"].reshape(N, K, 6)[..., 3:6].view(U) == 0).all() and (a["err"][:, 1].view(U) == 0).all() and (a["err"][:, 0] > 0).all()


@pytest.mark.parametrize("base", [False, True])
def test_a_target_out_of_reach_stays_bounded(host, base):
    """A target 3 m away: finite, every masked joint inside its limits, every update within max_step (q moves by at most I max_step, and by
    at most max_step with one iteration), converged 0 and iters = I."""
    for it in (1, 12):
        P = QR.problem(2, base=base, iterations=it, max_step=0.25)
        root, q0, tgt, _ = QR.case(N, 37, P)
        tgt[:, 0, 0:3] += np.array([3.0, 0.0, 0.0], F)
        tgt[:, 1, 0:3] += np.array([0.0, -2.0, 2.0], F)
        o = host_run(host, P, root, q0, tgt)
        assert all(np.isfinite(o[k]).all() for k in OUTS) and (o["converged"] == 0).all() and (o["iters"] == it).all()
        q = o["q"][:, P["dofs"]]
        assert (q >= QR.LOWER[P["dofs"]]).all() and (q <= QR.UPPER[P["dofs"]]).all()
        assert np.abs(o["q"] - q0).max() <= it * 0.25 * (1 + 1e-6)
        assert same(o["q"][:, ~P["dofs"]], q0[:, ~P["dofs"]])


def test_a_bad_target_spoils_its_env_only(host):
    """A NaN position, a zero quaternion, a quaternion of norm 1.02 and an infinite one: those envs' float outputs are NaN, their iters and
    converged 0; every other env keeps its bits.  A norm of 1.005 is normalised on the way in: the bits of the unit target, or within an ulp's
    effect."""
    P = QR.problem(2, iterations=5)
    root, q0, tgt, _ = QR.case(8, 41, P)
    o0 = host_run(host, P, root, q0, tgt)
    bad = tgt.copy()
    bad[1, 0, 1], bad[2, 1, 3:7], bad[4, 0, 3:7], bad[6, 1, 6] = np.nan, 0.0, bad[4, 0, 3:7] * F(1.02), np.inf
    bad[5, 0, 3:7] = bad[5, 0, 3:7] * F(1.005)
    o = host_run(host, P, root, q0, bad)
    for e in (1, 2, 4, 6):
        assert all(np.isnan(o[k][e]).all() for k in ("q", "root", "residual", "err")) and o["iters"][e] == 0 and o["converged"][e] == 0
    for k in OUTS:
        assert same(o[k][[0, 3, 7]], o0[k][[0, 3, 7]]), k
    assert np.isfinite(o["q"][5]).all() and np.abs(o["q"][5] - o0["q"][5]).max() < 1e-4


# ---------------------------------------------------------------------------------------------- 4. injected faults
@pytest.mark.parametrize("fault", QR.FAULTS)
def test_every_injected_fault_is_rejected(fault):
    """The float32 restatement passes the checks above; with a dropped row (the last active row never enters J and e), a dropped column (the
    last free column of J is zero) or a skipped clamp it does not: the one-step check rejects the first two, the limits check the third."""
    P = QR.problem(2, iterations=1)
    root, q0, tgt, _ = QR.case(N, 11, P)
    want = QR.step(root, q0, tgt, P)
    assert QR.within(QR.excess(QR.restate(root, q0, tgt, P), want, root, tgt, P))
    Pf = QR.problem(2, iterations=12, max_step=0.25)
    far = tgt.copy()
    far[:, 0, 0:3] += np.array([3.0, 0.0, 0.0], F)
    inside = lambda o: bool(((o["q"] >= QR.LOWER) & (o["q"] <= QR.UPPER))[:, Pf["dofs"]].all())          # noqa: E731
    assert inside(QR.restate(root, q0, far, Pf))
    if fault == "skip_clamp":
        assert not inside(QR.restate(root, q0, far, Pf, fault=fault))
    else:
        ex = QR.excess(QR.restate(root, q0, tgt, P, fault=fault), want, root, tgt, P)
        assert not QR.within(ex) and ex["q"] > 100, ex


# ---------------------------------------------------------------------------------------------- 5. the ABI
@pytest.fixture(scope="module")
def api():
    return cbind.declare(C.CDLL(build.build()), HEADER, "dwq_")


@pytest.mark.parametrize("check", ["prototypes", "layouts"])
def test_header_python_and_library_agree(check, tmp_path):
    import test_cbind as TC
    if check == "prototypes":
        TC.test_ctypes_prototypes_match_the_header(HEADER, "dwq_", "inverse_kinematics", C.CDLL(build.build()))
    else:
        TC.test_struct_layouts_match_the_host_compiler(HEADER, "dwq_", "inverse_kinematics", tmp_path)
    assert sorted(QM.EXPORTS) == ["abi_version", "last_error", "pack_table", "solve"]
    assert dict(build.SOURCES)[SRC] == ["-ffp-contract=off"] and "dw_inverse_kinematics.h" in build.HEADERS
    assert HEADER in open(os.path.join(ROOT, "isaacgymdyros_amd", "build.py")).read()          # (the staleness check's header list)
    K = QM.K
    assert K["DWQ_ABI_VERSION"] == 1 and (K["DWQ_NV"], K["DWQ_MAX_TARGETS"], K["DWQ_ROWS"], K["DWQ_MAX_ROWS"], K["DWQ_MAX_ITERATIONS"]) == (39, 4, 6, 24, 64)
    assert (K["DWQ_NUM_BODIES"], K["DWQ_NUM_DOF"], K["DWQ_MAX_TARGETS"]) == (CM.K["DWC_NUM_BODIES"], CM.K["DWC_NUM_DOF"], CM.K["DWC_MAX_CONTACTS"])
    assert K["DWQ_T_K"] == JM.K["DWJ_TABLE_WORDS"] and K["DWQ_T_TARGET"] == K["DWQ_T_K"] + 1 and K["DWQ_T_ROWS"] == K["DWQ_T_TARGET"] + 16
    assert K["DWQ_T_W"] == K["DWQ_T_ROWS"] + 1 and K["DWQ_T_DOFS"] == K["DWQ_T_W"] + 24 and K["DWQ_T_LIMIT"] == K["DWQ_T_DOFS"] + 2
    assert K["DWQ_T_PARAM"] == K["DWQ_T_LIMIT"] + 66 and K["DWQ_TABLE_WORDS"] == K["DWQ_T_PARAM"] + 6 and K["DWQ_TABLE_WORDS"] % 4 == 0
    assert "#define DWQ_MIN_DAMPING     4e-3f" in open(os.path.join(ROOT, "include", HEADER)).read()
    assert QM.DEFAULTS == {"targets": [{"body": "L_Foot_Link", "pos": [0.0, 0.0, -0.09]}, {"body": "R_Foot_Link", "pos": [0.0, 0.0, -0.09]}], "rows": None,
                           "weights": None, "dofs": None, "base": False, "iterations": 16, "damping": 0.05, "max_step": 0.5, "tol_pos": 1e-5, "tol_ang": 1e-5,
                           "limits": True, "target_frame": "world", "auto": False}
    from isaacgymdyros_amd import model_tensors as MT
    assert MT.SOLVERS == (("inverse_kinematics", "InverseKinematics", ()),)
    # no other symbol of the library begins with the prefix, and the older headers are untouched
    syms = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout.split()
    assert sorted(s for s in syms if s.startswith("dwq_")) == ["dwq_abi_version", "dwq_last_error", "dwq_pack_table", "dwq_solve"]
    assert CM.K["DWC_ABI_VERSION"] == 1 and JM.K["DWJ_ABI_VERSION"] == 1


def test_the_library_and_the_host_build_pack_the_same_table(host, api):
    japi = cbind.declare(C.CDLL(build.build()), "dyros_jacobians.h", "dwj_")
    capi = cbind.declare(C.CDLL(build.build()), "dyros_contact_dynamics.h", "dwc_")
    model = load_model()
    for K in (1, 2, 4):
        for base in (False, True):
            P = QR.problem(K, rows=QR.MIXED[K], weights=QR.ORI_10, base=base, iterations=7, damping=0.02, max_step=float("inf"), tol_pos=2e-5, tol_ang=3e-5,
                           limits=not base, rel_root=base)
            st, rm, w, dm, lo, hi, pr = table_args(P)
            t = QM.pack_table(api, model, st, None, rm, w, dm, lo, hi, pr)
            assert t.dtype == U and t.shape == (QM.TABLE_WORDS,) and np.array_equal(t, host_table(host, P))
            k = QM.K
            assert np.array_equal(t[:k["DWQ_T_K"]], JM.pack_table(japi, model)) and t[k["DWQ_T_K"]] == K
            c = CM.pack_table(capi, model, CR.ids_of(P["contacts"]), [p for _, p in P["contacts"]])
            assert np.array_equal(t[k["DWQ_T_TARGET"]:k["DWQ_T_ROWS"]], c[CM.K["DWC_T_CONTACT"]:CM.K["DWC_T_CONTACT"] + 16])
            assert t[k["DWQ_T_ROWS"]] == sum(1 << r for r in np.flatnonzero(P["rows"]))
            assert np.array_equal(t[k["DWQ_T_W"]:k["DWQ_T_W"] + 6 * K].view(F), P["w"]) and (t[k["DWQ_T_W"] + 6 * K:k["DWQ_T_DOFS"]] == 0).all()
            assert int(t[k["DWQ_T_DOFS"]]) | (int(t[k["DWQ_T_DOFS"] + 1]) << 32) == sum(1 << int(j) for j in np.flatnonzero(P["dofs"]))
            assert np.array_equal(t[k["DWQ_T_LIMIT"]:k["DWQ_T_PARAM"]].view(F).reshape(33, 2), np.stack([QR.LOWER, QR.UPPER], -1))
            prm = t[k["DWQ_T_PARAM"]:]
            assert prm[0] == 7 and np.array_equal(prm[1:5].view(F), np.array([0.02, np.inf, 2e-5, 3e-5], F)) and prm[5] == (1 | 4 if base else 2)
    # the defaults: every row, unit weights, every joint, the model's limits
    t = QM.pack_table(api, model, [8, 16], [[0, 0, -0.09]] * 2)
    assert t[QM.K["DWQ_T_ROWS"]] == 0xfff and t[QM.K["DWQ_T_DOFS"]] == 0xffffffff and t[QM.K["DWQ_T_DOFS"] + 1] == 1 and t[QM.K["DWQ_T_PARAM"]] == 16
    assert t[QM.K["DWQ_T_PARAM"] + 5] == 2 and np.array_equal(t[QM.K["DWQ_T_PARAM"] + 1:QM.K["DWQ_T_PARAM"] + 5].view(F), np.array([0.05, 0.5, 1e-5, 1e-5], F))
    # the default DoF mask is made on the Python side: the twelve leg joints for both feet
    assert QM.resolve(True)["dof_ids"] == QR.path_dofs(QR.SETS[2]) == list(range(12))
    assert QM.resolve({"targets": [{"body": n, "pos": list(p)} for n, p in QR.SETS[4]]})["dof_ids"] == QR.path_dofs(QR.SETS[4])


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_pack_table_refusals(api):
    model = load_model()
    feet, pos = [8, 16], [[0, 0, -0.09]] * 2
    bad = ((([], []), "count must be in 1..DWC_MAX_CONTACTS"), (([1, 2, 3, 4, 5], [[0, 0, 0]] * 5), "count must be in 1..DWC_MAX_CONTACTS"),
           (([8, 38], pos), "a body id is outside 0..37"), (([-1], pos[:1]), "a body id is outside 0..37"),
           ((feet, [[0, 0, -0.09], [0, float("nan"), 0]]), "pos is not finite"), (([8, 6], pos), "two contacts on one moving body"))
    for (ids, p), msg in bad:
        with pytest.raises(cbind.DyrosWalkLibraryError, match="dwq_pack_table: " + msg):
            QM.pack_table(api, model, ids, p)
    with pytest.raises(cbind.DyrosWalkLibraryError, match="dwq_pack_table: the row mask leaves no row active"):
        QM.pack_table(api, model, feet, pos, row_mask=np.zeros(12, np.uint8))
    for i, x in ((0, 0.0), (3, -1.0), (7, float("nan")), (11, float("inf"))):
        w = np.ones(12, F)
        w[i] = x
        with pytest.raises(cbind.DyrosWalkLibraryError, match=r"dwq_pack_table: a weight is not finite and positive \(index %d\)" % i):
            QM.pack_table(api, model, feet, pos, weights=w)
    for j, (lo, hi) in ((4, (0.5, 0.4)), (9, (float("nan"), 1.0)), (32, (-1.0, float("inf")))):
        a, b = QR.LOWER.copy(), QR.UPPER.copy()
        a[j], b[j] = lo, hi
        with pytest.raises(cbind.DyrosWalkLibraryError, match=r"dwq_pack_table: a joint limit is not finite, or lower > upper \(index %d\)" % j):
            QM.pack_table(api, model, feet, pos, lower=a, upper=b)
    for kw, msg in (({"iterations": 0}, "iterations must be in 1..DWQ_MAX_ITERATIONS"), ({"iterations": 65}, "iterations must be in 1..DWQ_MAX_ITERATIONS"),
                    ({"damping": 3.9e-3}, "damping must be in"), ({"damping": 0.0}, "damping must be in"), ({"damping": float("nan")}, "damping must be in"),
                    ({"damping": float("inf")}, "damping must be in"), ({"damping": 1.1e3}, "damping must be in"),
                    ({"max_step": 0.0}, "max_step must be positive"), ({"max_step": -1.0}, "max_step must be positive"), ({"max_step": float("nan")}, "max_step must be positive"),
                    ({"tol_pos": -1e-6}, "tol_pos and tol_ang"), ({"tol_ang": float("nan")}, "tol_pos and tol_ang"), ({"tol_ang": float("inf")}, "tol_pos and tol_ang")):
        with pytest.raises(cbind.DyrosWalkLibraryError, match="dwq_pack_table: " + msg):
            QM.pack_table(api, model, feet, pos, params=kw)
    for kw in ({"iterations": 1}, {"iterations": 64}, {"damping": 4e-3}, {"damping": 1e3}, {"max_step": float("inf")}, {"tol_pos": 0.0, "tol_ang": 0.0}):
        QM.pack_table(api, model, feet, pos, params=kw)
    for kw in ({"row_mask": np.ones(6, np.uint8)}, {"weights": np.ones(6, F)}, {"dof_mask": np.ones(32, np.uint8)}, {"lower": np.zeros(12, F)}):
        with pytest.raises(ValueError):
            QM.pack_table(api, model, feet, pos, **kw)
    # it refuses what dwj_pack_table refuses, under its own name
    d = {k: np.array(v) for k, v in model.d.items() if k in ("mv_parent", "mv_pos", "mv_rot0", "mv_axis", "body_moving", "inert_gym", "inert_mv", "inert_mass",
                                                             "inert_com", "inert_I", "dof_lower", "dof_upper")}
    d["mv_parent"][5] = 6
    with pytest.raises(cbind.DyrosWalkLibraryError, match="dwq_pack_table: a child precedes its parent"):
        QM.pack_table(api, d, feet, pos)
    t = np.zeros(QM.TABLE_WORDS, U)
    m, c, p = JM.model_struct(model), CM.contacts_struct(feet, pos), QM.params_struct(QM.DEFAULTS)
    ok = [C.byref(m), C.byref(c), None, None, None, QR.LOWER.ctypes.data, QR.UPPER.ctypes.data, C.byref(p), t.ctypes.data]
    assert api["pack_table"](*ok) == 0
    for i in (0, 1, 5, 6, 7, 8):
        args = list(ok)
        args[i] = None
        assert api["pack_table"](*args) == -1 and b"dwq_pack_table: a pointer is missing" in api["last_error"](), i


def test_refusals_happen_before_any_launch(api):
    """Every buffer is NULL or a host address here: a launch would fault, a refusal returns -1 with its message."""
    one = C.c_void_p(16)
    ok = lambda **kw: tuple(dict(dict(n=8, table=one, root=one, dof=one, q0=None, targets=one, q=one, root_out=None, residual=None, err=None, iters=None,          # noqa: E731
                                      converged=None, stream=None), **kw).values())
    for args, msg in ((ok(n=0), b"num_envs"), (ok(n=-3), b"num_envs"), (ok(n=1 << 30), b"num_envs"),
                      (ok(table=None), b"a buffer is missing"), (ok(root=None), b"a buffer is missing"), (ok(dof=None), b"a buffer is missing"),
                      (ok(targets=None), b"a buffer is missing"), (ok(table=C.c_void_p(8)), b"16-byte aligned"), (ok(table=C.c_void_p(20)), b"16-byte aligned"),
                      (ok(q=None), b"no output")):
        assert api["solve"](*args) == -1 and msg in api["last_error"]() and b"dwq_solve" in api["last_error"](), (args, api["last_error"]())


# ---------------------------------------------------------------------------------------------- 7. the kernel's resources
def test_kernel_uses_no_scratch_and_sixteen_envs_share_a_cu():
    """Exactly one kernel in the unit, dwq_k_solve: no scratch; its LDS is the table and per env the root row, the dof_state rows, the targets
    and the store of 1979 words -- 8.3 KB an env -- and four workgroups, 16 envs, share a CU's 160 KB at four waves per SIMD."""
    ks = RES.kernels(SRC)
    assert len(ks) == 1 and "dwq_k_solve" in next(iter(ks))
    r = next(iter(ks.values()))
    want = 4 * (QM.TABLE_WORDS + QM.GROUP * (13 + 66 + 28 + 1979))
    print("dwq_k_solve: %d VGPRs, scratch %d, LDS %d bytes per workgroup (%d an env), %d waves per SIMD" % (r["vgprs"], r["scratch"], r["lds"], (r["lds"] - 4 * QM.TABLE_WORDS) // QM.GROUP, r["occ"]))
    assert r["scratch"] == 0 and r["lds"] == want and r["lds"] <= 160 * 1024 // 4 and r["occ"] >= 4 and r["vgprs"] <= 128


# ---------------------------------------------------------------------------------------------- 8. the Python surface
def test_cfg_spec():
    assert QM.resolve(None) is None and QM.resolve(False) is None
    full = QM.resolve(True)
    assert full == QM.resolve({}) and {k: full[k] for k in QM.DEFAULTS} == QM.DEFAULTS and full["ids"] == [8, 16] and full["pos"] == [[0.0, 0.0, -0.09]] * 2
    assert full["w"] is None and full["row_mask"] == [1] * 12 and full["dof_ids"] == list(range(12)) and sum(full["dof_mask"]) == 12
    names = load_model().dof_names
    s = QM.resolve({"targets": [{"body": "base_link"}, {"body": 27, "pos": [0.1, 0, 0]}], "rows": ["orientation", "position"], "weights": [1, 1, 1, 10, 10, 10],
                    "dofs": [names[3], 20, 0], "base": True, "iterations": 64, "damping": 4e-3, "max_step": float("inf"), "tol_pos": 0, "tol_ang": 1e-3, "limits": False,
                    "target_frame": "root", "auto": True})
    assert s["ids"] == [0, 27] and s["row_mask"] == [0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0] and s["w"] == [1.0, 1.0, 1.0, 10.0, 10.0, 10.0] * 2 and s["dof_ids"] == [0, 3, 20]
    p = QM.params_struct(s)
    assert (p.iterations, p.free_base, p.clamp_limits, p.targets_rel_root) == (64, 1, 0, 1) and p.max_step == float("inf")
    foot = {"body": "L_Foot_Link"}
    for bad in (1, "on", ["targets"], {"h": True}, {"base": 1}, {"limits": None}, {"auto": "no"}, {1: True},
                {"weights": 1.0}, {"weights": [1] * 5}, {"weights": [1, 1, 1, 1, 1, 0]}, {"weights": [[1] * 6]},
                {"rows": "pose"}, {"rows": ["pose"]}, {"rows": ["pose", "twist"]}, {"rows": ["pose", 1]}, {"rows": ["pose"] * 3},
                {"dofs": []}, {"dofs": "L_Knee_Joint"}, {"dofs": [33]}, {"dofs": [-1]}, {"dofs": ["no_such_joint"]}, {"dofs": [1, 1]}, {"dofs": [True]},
                {"iterations": 0}, {"iterations": 65}, {"iterations": 2.0}, {"iterations": True}, {"damping": 3e-3}, {"damping": 2e3}, {"damping": float("nan")},
                {"damping": "0.05"}, {"max_step": 0}, {"max_step": -0.5}, {"max_step": float("nan")}, {"tol_pos": -1e-9}, {"tol_ang": float("inf")}, {"tol_pos": None},
                {"target_frame": "base"}, {"target_frame": None},
                {"targets": []}, {"targets": "L_Foot_Link"}, {"targets": [foot] * 5}, {"targets": [{"pos": [0, 0, 0]}]}, {"targets": [{"body": "no_such_link"}]},
                {"targets": [{"body": 38}]}, {"targets": [{"body": 8, "pos": [0, 0]}]}, {"targets": [foot, {"body": "L_AnkleRoll_Link"}]}):
        with pytest.raises(ValueError):
            QM.resolve(bad)
    with pytest.raises(ValueError, match="inverse_kinematics.targets"):
        QM.resolve({"targets": [{"body": "no_such_link"}]})
    from isaacgymdyros_amd.config import default_cfg, validate_cfg
    cfg = default_cfg(64, "cpu")
    assert "inverse_kinematics" not in cfg["sim"]["mi355"] and "amp_inverse_kinematics" not in cfg["sim"]["mi355"]          # (off by default)
    for key in ("inverse_kinematics", "amp_inverse_kinematics"):
        cfg = default_cfg(64, "cpu")
        cfg["sim"]["mi355"][key] = {"rows": ["position", "pose"], "base": True, "auto": True}
        validate_cfg(cfg)
        cfg["sim"]["mi355"][key] = True
        validate_cfg(cfg)
        for bad in ({"mass": True}, {"base": 1}, {"weights": [1] * 7}, {"damping": 0}, "on", {"targets": [foot, foot]}):
            cfg["sim"]["mi355"][key] = bad
            with pytest.raises(ValueError):
                validate_cfg(cfg)
    # TocabiAMPLower keeps its own key from the physics host
    src = open(os.path.join(ROOT, "isaacgymdyros_amd", "tocabi_amp_lower.py")).read()
    assert re.search(r'k not in \([^)]*"amp_inverse_kinematics"[^)]*\)', src)
