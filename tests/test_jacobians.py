"""The Jacobian and mass-matrix tensors without a GPU (include/dyros_jacobians.h, isaacgymdyros_amd/csrc/dw_jacobian.h):
the header, the Python binding and the built library agree; refusals; the kernels' resources; the reference (tests/jacobians_ref.py) against
things that are not itself; the per-env arithmetic -- compiled by g++ from the header the HIP kernels include (tests/jacobians_host.cpp) --
against the float64 reference under its measured tolerance; the outputs' exact properties; the cfg surface."""
import copy
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import body_states_ref as R
import jacobians_ref as JR
from isaacgymdyros_amd import build, cbind
from isaacgymdyros_amd import jacobians as JM
from isaacgymdyros_amd.model import load_model
from test_body_states import TAKEN as TAKEN_BODIES          # noqa: F401  (the tuple of test_gait_profile_abi, re-exported there)
from test_gait_profile_abi import TAKEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dw_jacobian.hip"
N = 37
SUBSET = [37, 0, 16, 8, 8]
F = np.float32
U = np.uint32


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------- 1. the ABI
@pytest.fixture(scope="module")
def api():
    return cbind.declare(C.CDLL(build.build()), "dyros_jacobians.h", "dwj_")


@pytest.mark.parametrize("check", ["prototypes", "layouts"])
def test_header_python_and_library_agree(check, tmp_path):
    import test_cbind as TC
    if check == "prototypes":
        TC.test_ctypes_prototypes_match_the_header("dyros_jacobians.h", "dwj_", "jacobians", C.CDLL(build.build()))
    else:
        TC.test_struct_layouts_match_the_host_compiler("dyros_jacobians.h", "dwj_", "jacobians", tmp_path)
    assert sorted(JM.EXPORTS) == ["abi_version", "jacobian", "last_error", "mass_matrix", "pack_table"]
    assert dict(build.SOURCES)[SRC] == ["-ffp-contract=off"] and "dw_jacobian.h" in build.HEADERS
    K, KB = JM.K, cbind.constants("dyros_bodies.h", "dwb_")
    assert K["DWJ_ABI_VERSION"] == 1 and (K["DWJ_NV"], K["DWJ_JAC_ROWS"]) == (39, 6)
    for name in ("NUM_BODIES", "NUM_MOVING", "NUM_DOF", "NUM_INERT"):
        assert K["DWJ_" + name] == KB["DWB_" + name]
    assert K["DWJ_T_ANC"] == KB["DWB_TABLE_WORDS"] and K["DWJ_T_SUB"] == K["DWJ_T_ANC"] + 68 and K["DWJ_T_I"] == K["DWJ_T_SUB"] + 68
    assert K["DWJ_TABLE_WORDS"] == K["DWJ_T_I"] + 216 and K["DWJ_TABLE_WORDS"] % 4 == 0
    assert K["DWJ_GROUP"] * K["DWJ_LANES"] == 256
    assert C.sizeof(JM.DwjModel) == 4 * (34 * 16 + 38 + 36 * 6 + 36 * 6)
    # the older headers are untouched
    assert KB["DWB_ABI_VERSION"] == 1 and cbind.constants("dyros_walk.h", "dw_")["DW_ABI_VERSION"] >= 1


def test_refusals_happen_before_any_launch(api):
    """Every buffer is NULL or a host address here: a launch would fault, a refusal returns -1 with its message."""
    one = C.c_void_p(16)
    ids = (C.c_int32 * 2)(0, 38)
    for args, msg in (((0, one, one, one, None, 0, 0, one, None), b"num_envs"),
                      ((-3, one, one, one, None, 0, 0, one, None), b"num_envs"),
                      ((8, None, one, one, None, 0, 0, one, None), b"a buffer is missing"),
                      ((8, one, None, one, None, 0, 0, one, None), b"a buffer is missing"),
                      ((8, one, one, None, None, 0, 0, one, None), b"a buffer is missing"),
                      ((8, one, one, one, None, 0, 0, None, None), b"a buffer is missing"),
                      ((8, one, one, one, None, 5, 0, one, None), b"nb must be 0 or 38"),
                      ((8, one, one, one, ids, 0, 0, one, None), b"nb must be in 1..38"),
                      ((8, one, one, one, ids, 39, 0, one, None), b"nb must be in 1..38"),
                      ((8, one, one, one, ids, 2, 0, one, None), b"outside 0..37"),
                      ((8, C.c_void_p(4), one, one, None, 0, 0, one, None), b"16-byte aligned")):
        assert api["jacobian"](*args) == -1 and msg in api["last_error"]() and b"dwj_jacobian" in api["last_error"](), (args, api["last_error"]())
    for args, msg in (((0, one, one, one, None, None, 0, one, None, None), b"num_envs"),
                      ((8, None, one, one, None, None, 0, one, None, None), b"a buffer is missing"),
                      ((8, one, None, one, None, None, 0, one, None, None), b"a buffer is missing"),
                      ((8, one, one, None, None, None, 0, one, None, None), b"a buffer is missing"),
                      ((8, one, one, one, None, None, 0, None, one, None), b"a buffer is missing"),
                      ((8, C.c_void_p(8), one, one, None, None, 0, one, None, None), b"16-byte aligned")):
        assert api["mass_matrix"](*args) == -1 and msg in api["last_error"]() and b"dwj_mass_matrix" in api["last_error"](), (args, api["last_error"]())


def test_pack_table_validates_the_model(api):
    d = load_model().d
    t = JM.pack_table(api, d)
    K = JM.K
    assert t.dtype == U and t.shape == (K["DWJ_TABLE_WORDS"],)
    from isaacgymdyros_amd import body_states as B
    tb = B.pack_table(cbind.declare(C.CDLL(build.build()), "dyros_bodies.h", "dwb_"), d)
    assert np.array_equal(t[:K["DWJ_T_ANC"]], tb)          # the chain's table, word for word
    anc = t[K["DWJ_T_ANC"]:K["DWJ_T_SUB"]].reshape(34, 2)
    sub = t[K["DWJ_T_SUB"]:K["DWJ_T_I"]].reshape(34, 2)
    for m in range(34):
        bits = [b for b in range(64) if (int(anc[m, b >> 5]) >> (b & 31)) & 1]
        assert bits == sorted(JR.ANC[m]), m
        recs = [k for k in range(64) if (int(sub[m, k >> 5]) >> (k & 31)) & 1]
        assert recs == [k for k in range(36) if m == 0 or m in JR.ANC[R.INERT_MV[k]]], m          # (ANC holds the body itself, not the base)
    assert [k for k in range(64) if (int(sub[0, k >> 5]) >> (k & 31)) & 1] == list(range(36))
    I6 = t[K["DWJ_T_I"]:].view(F).reshape(36, 6)
    I = np.asarray(d["inert_I"], np.float64)
    assert np.array_equal(I6, np.stack([I[:, 0, 0], I[:, 1, 1], I[:, 2, 2], I[:, 0, 1], I[:, 0, 2], I[:, 1, 2]], 1).astype(F))

    def refused(msg, **change):
        bad = copy.deepcopy({k: d[k] for k in ("mv_parent", "mv_pos", "mv_rot0", "mv_axis", "body_moving", "inert_gym", "inert_mv", "inert_mass", "inert_com", "inert_I")})
        for k, (i, v) in change.items():
            bad[k][i] = v
        with pytest.raises(cbind.DyrosWalkLibraryError, match=msg):
            JM.pack_table(api, bad)
    refused("dwj_pack_table: a child precedes its parent", mv_parent=(5, 6))
    refused("mv_parent out of range", mv_parent=(5, 34))
    refused("body_moving out of range", body_moving=(7, 34))
    refused("body_moving out of range", body_moving=(7, -1))
    refused("inert_gym out of range", inert_gym=(3, 38))
    refused("inert_mv out of range", inert_mv=(3, -2))
    refused("two inertial records", inert_gym=(7, 6))
    refused("not its Gym body's carrier", inert_mv=(3, 4))
    refused("inert_I is not finite", inert_I=(9, [[1.0, 0.0, 0.0], [0.0, float("nan"), 0.0], [0.0, 0.0, 1.0]]))
    refused("inert_I is not finite", inert_I=(35, [[1.0, 0.0, float("inf")], [0.0, 1.0, 0.0], [float("inf"), 0.0, 1.0]]))


# ---------------------------------------------------------------------------------------------- 2. the kernels' resources
@pytest.fixture(scope="module")
def remarks():
    extra = dict(build.SOURCES)[SRC]
    cmd = [build.hipcc()] + build.FLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(build.CSRC, SRC)]
    return subprocess.run(cmd, cwd=build.CSRC, capture_output=True, text=True, check=True).stderr


def test_kernels_use_no_scratch_and_fit_the_lds(remarks):
    names = re.findall(r"remark: Function Name: (\S+)", remarks)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)]
    assert len(names) == 2 and len(scratch) == len(lds) == len(names)
    assert any("dwj_k_jacobian" in n for n in names) and any("dwj_k_mass_matrix" in n for n in names)
    for n, s, l in zip(names, scratch, lds):
        assert "dwj_k_" in n and s == 0 and l <= 65536, (n, s, l)
        assert not any(x in n for x in tuple(TAKEN) + tuple(TAKEN_BODIES) + ("dwg_k_", "dwb_k_")), n


# ---------------------------------------------------------------------------------------------- 3. the reference against what is not itself
@pytest.fixture(scope="module")
def ref8():
    """8 states in both modes: float64 chain, Jacobian, M without armature."""
    root, dof, ms = R.states(8, 5, mass=True)
    out = {"root": root, "dof": dof, "ms": ms}
    for v in (0, 1):
        c = R.chain(root, dof, np.float64, v)
        M, tot = JR.mass_matrix(c, v, ms)
        out[v] = {"c": c, "J": JR.jacobian(c, v), "M": M, "tot": tot}
    return out


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_reference_jacobian_times_nu_is_the_body_velocity(ref8, vel_at_com):
    r = ref8[vel_at_com]
    nu = JR.nu(ref8["root"], ref8["dof"])
    rows = R.rows(r["c"], vel_at_com)
    err = np.abs(np.einsum("nkic,nc->nki", r["J"], nu) - np.concatenate([rows["vel"], rows["w"]], -1)).max()
    # the COM Jacobian against body_states_ref.com, and the energy against the records' own velocities
    co = R.com(r["c"], ref8["ms"])
    ec = np.abs(np.einsum("nic,nc->ni", r["M"][:, 0:3] / r["tot"][:, None, None], nu) - co[1]).max()
    ke = JR.kinetic_energy(r["c"], vel_at_com, ref8["ms"])
    ee = np.abs(0.5 * np.einsum("na,nab,nb->n", nu, r["M"], nu) / ke - 1).max()
    print("J nu %.1e m/s, com_jacobian nu %.1e m/s, energy %.1e (relative)" % (err, ec, ee))
    assert err < 1e-12 and ec < 1e-12 and ee < 1e-12
    assert np.abs(r["tot"] - co[2]).max() < 1e-12 and np.abs(r["M"] - np.swapaxes(r["M"], 1, 2)).max() < 1e-12
    assert (r["J"][:, ~np.broadcast_to(JR.dof_mask()[:, None, :], (38, 6, 39))] == 0).all() and (r["M"][:, ~JR.branch_mask()] == 0).all()


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_reference_jacobian_columns_are_derivatives_of_its_poses(vel_at_com):
    """Central differences, h = 1e-6, of body_states_ref's own poses under a unit velocity in each of the 39 coordinates, at 64 states.  The
    bound, 1e-7, is a tenth of the float32 restatement's d for the Jacobian's entries (1.2e-6 to 1.5e-6), so the reference's own error cannot
    eat the margin of four.  What to expect: truncation h^2 / 6 times a third derivative of order 10, about 2e-12, and rounding 2^-52 |x| / h,
    about 2e-10 per term of an 11-deep sum."""
    h = 1e-6
    root, dof, _ = R.states(64, 71)
    root, dof = root.astype(np.float64), dof.astype(np.float64)
    c = R.chain(root, dof, np.float64, vel_at_com)
    J = JR.jacobian(c, vel_at_com)
    carriers, p = JR.points(c, vel_at_com)
    pr = JR.p_ref(c, vel_at_com)
    local = [None] * 38          # the rows' points in their carriers' frames
    for g in range(38):
        local[g] = np.einsum("nji,nj->ni", c["R"][:, carriers[g]], p[:, g] - c["off"][:, carriers[g]])

    def posed(col, s):
        """The rows' points (absolute) and rotations after s * h of unit velocity in coordinate col."""
        r2, d2 = root.copy(), dof.copy()
        if col < 3:
            r2[:, col] += s * h
        elif col < 6:
            # a rotation about world axis col - 3 through the reference point: the reference point stays, the base origin swings about it
            a = np.zeros(3)
            a[col - 3] = 1.0
            dq = np.concatenate([a * np.sin(s * h / 2), [np.cos(s * h / 2)]])
            r2[:, 3:7] = R.qmul(np.broadcast_to(dq, (len(root), 4)), root[:, 3:7])
            Rd = R.qmat(dq[None])[0]
            r2[:, 0:3] = root[:, 0:3] + pr - pr @ Rd.T
        else:
            d2[:, col - 6, 0] += s * h
        c2 = R.chain(r2, d2)
        x = np.stack([r2[:, 0:3] + c2["off"][:, carriers[g]] + R.mv3(c2["R"][:, carriers[g]], local[g]) for g in range(38)], 1)
        return x, c2["R"][:, carriers]
    worst = 0.0
    for col in range(39):
        (xp, Rp), (xm, Rm) = posed(col, +1.0), posed(col, -1.0)
        lin = (xp - xm) / (2 * h)
        W = ((Rp - Rm) / (2 * h)) @ np.swapaxes(c["R"][:, carriers], -1, -2)
        ang = np.stack([W[..., 2, 1], W[..., 0, 2], W[..., 1, 0]], -1)
        worst = max(worst, float(np.abs(J[..., 0:3, col] - lin).max()), float(np.abs(J[..., 3:6, col] - ang).max()))
    print("finite differences of the poses against the Jacobian's columns: %.2e" % worst)
    assert worst < 1e-7


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_reference_mass_matrix_is_congruent_to_the_dense_dynamics(ref8, vel_at_com):
    """M == T' M_dense T, M_dense = tests/dense_dynamics_np.py DenseDynamics.terms(...)["M"] with zero armature (world-origin spatial vectors, a
    base twist in base coordinates): T maps nu to [R0' w, R0' (v_ref - w x R0 c0), qdot]."""
    from dense_dynamics_np import DenseDynamics, skew
    model = load_model()
    dd = DenseDynamics(model)
    root, dof, ms = (ref8[k].astype(np.float64) for k in ("root", "dof", "ms"))
    worst, big = 0.0, 0.0
    for e in range(8):
        t = dd.terms(root[e, 0:3], root[e, 3:7], dof[e, :, 0], np.zeros(6), np.zeros(33), ms[e], np.zeros(33), np.zeros(33), 0.0, np.zeros(3), np.zeros(33))
        R0 = t["Rw"][0]
        c0 = np.asarray(model.inert_com[R.RECORD[0]], np.float64) if vel_at_com else np.zeros(3)
        T = np.zeros((39, 39))
        T[0:3, 3:6] = R0.T
        T[3:6, 0:3] = R0.T
        T[3:6, 3:6] = R0.T @ skew(R0 @ c0)          # -(w x r) = r x w = [r]x w
        T[6:, 6:] = np.eye(33)
        worst = max(worst, float(np.abs(T.T @ t["M"] @ T - ref8[vel_at_com]["M"][e]).max()))
        big = max(big, float(np.abs(t["M"]).max()))
    print("congruence with the dense dynamics: %.2e on entries up to %.0f" % (worst, big))
    assert worst < 1e-11


# ---------------------------------------------------------------------------------------------- 4. the g++ build against float64
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/jacobians_host.cpp")
    so = str(tmp_path_factory.mktemp("dwjh") / "libdwjh.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, os.path.join(ROOT, "tests", "jacobians_host.cpp")])
    lib = C.CDLL(so)
    lib.dwjh_jacobian.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p]
    lib.dwjh_mass_matrix.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 2
    lib.dwjh_pack_table.argtypes = [C.POINTER(JM.DwjModel), C.c_void_p, C.c_char_p, C.c_int]
    table, err = np.zeros(JM.TABLE_WORDS, U), C.create_string_buffer(256)
    m = JM.model_struct(load_model())
    assert lib.dwjh_pack_table(C.byref(m), _p(table), err, 256) == 0, err.value
    lib.table = table
    return lib


def host_jac(lib, root, dof, vel_at_com, ids=None):
    n, nb = len(root), 38 if ids is None else len(ids)
    J = np.full((n, nb, 6, 39), np.nan, F)
    arr = None if ids is None else np.asarray(ids, np.int32)
    assert lib.dwjh_jacobian(n, _p(lib.table), _p(root), _p(dof), _p(arr), nb, vel_at_com, _p(J)) == 0
    return J


def host_mm(lib, root, dof, ms, arm, vel_at_com, cj=True):
    n = len(root)
    M, CJ = np.full((n, 39, 39), np.nan, F), np.full((n, 3, 39), np.nan, F) if cj else None
    assert lib.dwjh_mass_matrix(n, _p(lib.table), _p(root), _p(dof), _p(ms), _p(arm), vel_at_com, _p(M), _p(CJ)) == 0
    return M, CJ


def test_the_library_and_the_host_build_pack_the_same_table(api, host):
    assert np.array_equal(JM.pack_table(api, load_model()), host.table)


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_host_build_against_float64(host, vel_at_com):
    root, dof, ms = R.states(N, 11 + vel_at_com, mass=True)
    arm = JR.armature_of(N, 12)
    J = host_jac(host, root, dof, vel_at_com)
    M, CJ = host_mm(host, root, dof, ms, arm, vel_at_com)
    ex = JR.excess(root, dof, ms, arm, vel_at_com, J, M, CJ, report="host N=%d vel_at_com=%d" % (N, vel_at_com))
    assert JR.within(ex), ex
    # without mass scale and armature
    M1, CJ1 = host_mm(host, root, dof, None, None, vel_at_com)
    ex = JR.excess(root, dof, None, None, vel_at_com, None, M1, CJ1, report="host, nominal masses, no armature")
    assert JR.within(ex), ex
    assert np.array_equal(np.diagonal(M, axis1=1, axis2=2)[:, :6].view(U), np.diagonal(host_mm(host, root, dof, ms, None, vel_at_com)[0], axis1=1, axis2=2)[:, :6].view(U))
    # the energy: nu' M nu / 2 against the records' own velocities, within what the entry allowances imply
    nu = JR.nu(root, dof)
    c = R.chain(root, dof, np.float64, vel_at_com)
    Mn = host_mm(host, root, dof, ms, None, vel_at_com, cj=False)[0].astype(np.float64)
    allow = 0.5 * np.einsum("na,ab,nb->n", np.abs(nu), JR.allowance(vel_at_com), np.abs(nu))
    err = np.abs(0.5 * np.einsum("na,nab,nb->n", nu, Mn, nu) - JR.kinetic_energy(c, vel_at_com, ms))
    print("energy: %.2e J off at most, %.3f of the allowance" % (err.max(), (err / allow).max()))
    assert (err <= allow).all()


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_exact_properties(host, vel_at_com):
    root, dof, ms = R.states(N, 21, mass=True)
    arm = JR.armature_of(N, 22)
    J = host_jac(host, root, dof, vel_at_com)
    M, CJ = host_mm(host, root, dof, ms, arm, vel_at_com)
    assert np.isfinite(J).all() and np.isfinite(M).all() and np.isfinite(CJ).all()
    assert np.array_equal(M.view(U), np.swapaxes(M, 1, 2).view(U))                                             # symmetric bit for bit
    mask = np.broadcast_to(JR.dof_mask()[:, None, :], (38, 6, 39))
    assert (J.view(U)[:, ~mask] == 0).all() and (M.view(U)[:, ~JR.branch_mask()] == 0).all()              # +0.0, not -0.0
    assert np.array_equal(mask[:, 0], JM.dof_mask(list(range(38)), load_model()))
    eye = np.zeros((6, 39), F)
    eye[np.arange(6), np.arange(6)] = 1
    assert np.array_equal(J[:, 0].view(U), np.broadcast_to(eye, (N, 6, 39)).view(U))                         # row 0 is [I 0; 0 I | 0]
    # the base block of every row: identities and exact zeros around -[p - p_ref]x
    assert np.array_equal(J[:, :, 0:3, 0:3].view(U), np.broadcast_to(eye[0:3, 0:3], (N, 38, 3, 3)).view(U))
    assert np.array_equal(J[:, :, 3:6, 0:6].view(U), np.broadcast_to(eye[3:6, 0:6], (N, 38, 3, 6)).view(U))
    assert (J[:, :, [0, 1, 2], [3, 4, 5]].view(U) == 0).all()
    # the welded foot bodies: the angular rows are the carrier's
    for carrier, welded in ((6, (7, 8)), (14, (15, 16))):
        for g in welded:
            assert np.array_equal(J[:, g, 3:6].view(U), J[:, carrier, 3:6].view(U))
            if not vel_at_com:
                assert np.array_equal(J[:, g].view(U), J[:, carrier].view(U))
    # a subset with a repeat: the full tensor's rows bit for bit
    sub = host_jac(host, root, dof, vel_at_com, ids=SUBSET)
    assert np.array_equal(sub.view(U), J[:, SUBSET].view(U))
    # the mass matrix' base block: the total mass on the diagonal of the linear block, and the COM Jacobian's first block is the identity
    assert np.array_equal(CJ[:, :, 0:3].view(U), np.broadcast_to(eye[0:3, 0:3], (N, 3, 3)).view(U))
    # 640 m out: the same bits
    far = root.copy()
    far[:, 0:2] += np.array([640.0, -640.0], F)
    assert np.array_equal(host_jac(host, far, dof, vel_at_com).view(U), J.view(U))
    Mf, CJf = host_mm(host, far, dof, ms, arm, vel_at_com)
    assert np.array_equal(Mf.view(U), M.view(U)) and np.array_equal(CJf.view(U), CJ.view(U))
    # velocities do not enter
    still_r, still_d = root.copy(), dof.copy()
    still_r[:, 7:13], still_d[:, :, 1] = 0, 0
    assert np.array_equal(host_jac(host, still_r, still_d, vel_at_com).view(U), J.view(U))


def test_non_finite_inputs_stay_in_their_env(host):
    root, dof, ms = R.states(5, 41, mass=True)
    J0, (M0, C0) = host_jac(host, root, dof, 1), host_mm(host, root, dof, ms, None, 1)
    root[2, 4], dof[3, 20, 0] = np.nan, np.inf
    J, (M, CJ) = host_jac(host, root, dof, 1), host_mm(host, root, dof, ms, None, 1)
    keep = [0, 1, 4]
    for a, b in ((J, J0), (M, M0), (CJ, C0)):
        assert np.array_equal(a[keep].view(U), b[keep].view(U))
    assert np.isnan(J[2, 1:, :, 6:]).any() and np.isnan(M[2]).any() and np.isnan(CJ[2]).any()
    assert np.isnan(J[3, 27]).any() and np.isnan(M[3]).any()
    # the structural zeros and the base's own row are stored whatever the state holds
    mask = np.broadcast_to(JR.dof_mask()[:, None, :], (38, 6, 39))
    assert (J.view(U)[:, ~mask] == 0).all() and np.isfinite(J[:, 0]).all()


# ---------------------------------------------------------------------------------------------- 5. the Python surface
def test_cfg_spec_and_selection():
    full = {"bodies": None, "jacobian": True, "mass_matrix": True, "com_jacobian": False, "armature": True, "auto": False, "ids": list(range(38))}
    assert JM.resolve(None) is None and JM.resolve(False) is None
    assert JM.resolve(True) == JM.resolve({}) == full
    s = JM.resolve({"bodies": ["Head_Link", 8, "R_Foot_Link", 8], "com_jacobian": True, "auto": True, "armature": False})
    assert s["ids"] == [29, 8, 16, 8] and s["com_jacobian"] is True and s["auto"] is True and s["armature"] is False
    assert JM.resolve({"jacobian": False})["mass_matrix"] is True and JM.resolve({"mass_matrix": False})["jacobian"] is True
    for bad in (1, "on", [8], {"body": [8]}, {"bodies": []}, {"bodies": [38]}, {"bodies": [-1]}, {"bodies": ["Tail_Link"]}, {"bodies": "Head_Link"},
                {"bodies": [True]}, {"bodies": list(range(38)) + [0]}, {"com_jacobian": 1}, {"auto": "yes"}, {"armature": None}, {"jacobian": 0},
                {"com": True}, {"jacobian": False, "mass_matrix": False}, {"mass_matrix": False, "com_jacobian": True}):
        with pytest.raises(ValueError):
            JM.resolve(bad)
    with pytest.raises(ValueError, match="jacobians.bodies"):
        JM.resolve({"bodies": ["Tail_Link"]})
    m = JM.dof_mask([29, 8, 0], load_model())
    names = load_model().dof_names
    assert m.shape == (3, 39) and m[:, 0:6].all() and not m[2, 6:].any()
    assert [names[j] for j in np.flatnonzero(m[1, 6:])] == names[0:6]          # the left foot: the six left-leg joints
    assert m[0, 6:].sum() == 5 and m[1, 6:].sum() == 6
    from isaacgymdyros_amd.config import default_cfg, validate_cfg
    cfg = default_cfg(64, "cpu")
    assert "jacobians" not in cfg["sim"]["mi355"] and "amp_jacobians" not in cfg["sim"]["mi355"]          # (off by default)
    for key in ("jacobians", "amp_jacobians"):
        cfg = default_cfg(64, "cpu")
        cfg["sim"]["mi355"][key] = {"bodies": ["Head_Link", "L_Foot_Link", "R_Foot_Link"], "com_jacobian": True}
        validate_cfg(cfg)
        cfg["terrain"] = dict(cfg.get("terrain") or {})          # nothing here depends on terrain: the key is accepted beside any terrain cfg
        validate_cfg(cfg)
        cfg["sim"]["mi355"][key] = {"bodies": ["Head"]}
        with pytest.raises(ValueError):
            validate_cfg(cfg)
        cfg["sim"]["mi355"][key] = {"mass": True}
        with pytest.raises(ValueError):
            validate_cfg(cfg)
