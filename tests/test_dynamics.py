"""The bias-force, gravity, inverse-dynamics and momentum tensors without a GPU (include/dyros_dynamics.h, isaacgymdyros_amd/csrc/dw_dynamics.h,
DESIGN.md section 24): the reference (tests/dynamics_ref.py) against things that are not itself -- the mass matrix, central differences of the
chain's own velocities, the power balance, the centre of mass, the dense dynamics' momentum and forward dynamics; the per-env arithmetic --
compiled by g++ from the header the HIP kernel includes (tests/dynamics_host.cpp) -- against the float64 reference under its measured
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
import dynamics_ref as DR
import jacobians_ref as JR
from isaacgymdyros_amd import build, cbind
from isaacgymdyros_amd import dynamics as DM
from isaacgymdyros_amd import jacobians as JM
from isaacgymdyros_amd.model import load_model
from test_body_states import TAKEN as TAKEN_BODIES          # noqa: F401  (the tuple of test_gait_profile_abi, re-exported there)
from test_gait_profile_abi import TAKEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dw_dynamics.hip"
N = 37
F = np.float32
U = np.uint32
OUTS = ("bias", "gravity", "tau", "momentum")
G64 = np.asarray(DR.GRAVITY, F).astype(np.float64)
cross = R.cross


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------- 1. the reference against what is not itself
@pytest.fixture(scope="module")
def ref8():
    """8 seeded states in float64, both modes: chain, outputs (with armature and accel), M with armature."""
    root, dof, ms, arm, acc = DR.seeded(8, 5)
    out = {"root": root.astype(np.float64), "dof": dof.astype(np.float64), "ms": ms, "arm": arm, "acc": acc.astype(np.float64)}
    for v in (0, 1):
        c = R.chain(root, dof, np.float64, v)
        M, tot = JR.mass_matrix(c, v, ms, arm)
        out[v] = {"c": c, "out": DR.evaluate(root, dof, v, ms, arm, out["acc"], c=c), "M": M, "tot": tot}
    return out


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_reference_is_linear_in_the_acceleration(ref8, vel_at_com):
    """tau(a) - h == M a with jacobians_ref's dense mass matrix, in float64 at round-off: 39 products of |M| <= 100 and |a| <= 200 per row."""
    r = ref8[vel_at_com]
    want = np.einsum("nab,nb->na", r["M"], ref8["acc"])
    err = np.abs(r["out"]["tau"] - r["out"]["bias"] - want)
    allow = 64 * 2.0 ** -52 * (np.einsum("nab,nb->na", np.abs(r["M"]), np.abs(ref8["acc"])) + np.abs(r["out"]["bias"]))
    print("tau - h against M a: %.2e on values up to %.0f, %.3f of the round-off allowance" % (err.max(), np.abs(want).max(), (err / allow).max()))
    assert (err <= allow).all()


def advanced(root, dof, acc, pr, s, h):
    """The float64 state after s * h of (nu, a): q + s h qd, nu + s h a, the base attitude by the exponential of s h omega, p_ref by s h v."""
    r2, d2 = root.copy(), dof.copy()
    d2[:, :, 0] += s * h * dof[:, :, 1]
    d2[:, :, 1] += s * h * acc[:, 6:]
    r2[:, 7:13] += s * h * acc[:, 0:6]
    w = root[:, 10:13]
    ang = np.linalg.norm(w, axis=1, keepdims=True)
    dq = np.concatenate([w / ang * np.sin(s * h * ang / 2), np.cos(s * h * ang / 2)], 1)
    r2[:, 3:7] = R.qmul(dq, root[:, 3:7])
    pr2 = np.einsum("nij,nj->ni", R.qmat(dq), pr)          # p_ref turns with the base
    r2[:, 0:3] = root[:, 0:3] + pr + s * h * root[:, 7:10] - pr2
    return r2, d2


def com_velocities(c):
    """The records' COM velocities and their carriers' angular velocities [N, 36, 3], from the chain's own velocity words."""
    om = c["w"][:, R.INERT_MV]
    Rm = c["R"][:, R.INERT_MV]
    d = np.stack([R.mv3(Rm[:, k], R.INERT_COM[k]) for k in range(R.NI)], 1)
    return c["vo"][:, R.INERT_MV] + cross(om, d), om


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_reference_against_central_differences(vel_at_com):
    """cdd_k and alpha_m by central differences, h = 1e-6, of body_states_ref's own velocities along (nu, a) at 64 seeded states -- no recursion
    formula for accelerations -- assembled through the dense Jacobians.  The bound, 1e-4 N or N m, is a twentieth of the float32
    restatement's d for tau (1.6e-3 to 2.4e-3), so the reference's own error cannot eat the margin of four.  What to expect: truncation
    h^2 / 6 times a third derivative of a COM velocity (omega^3 |v|, omega a r: up to 1e5 m/s^4), 2e-8 m/s^2, and rounding 2^-52 |v| / h, 4e-9 m/s^2,
    each times a weight of up to 20 kg and summed over 36 records through Jacobian entries of order one: 1e-5 at the worst."""
    h, n = 1e-6, 64
    root, dof, ms, arm, acc = DR.seeded(n, 71)
    root, dof, acc = root.astype(np.float64), dof.astype(np.float64), acc.astype(np.float64)
    c = R.chain(root, dof, np.float64, vel_at_com)
    ref = DR.evaluate(root, dof, vel_at_com, ms, arm, acc, c=c)
    pr = JR.p_ref(c, vel_at_com)
    (vp, wp), (vm, wm) = (com_velocities(R.chain(*advanced(root, dof, acc, pr, s, h), np.float64, vel_at_com)) for s in (1.0, -1.0))
    cdd, al = (vp - vm) / (2 * h), (wp - wm) / (2 * h)
    w, pc, Iw = JR.records(c, ms)
    om = c["w"][:, R.INERT_MV]
    f = w[..., None] * (cdd - G64)
    nk = np.einsum("nkij,nkj->nki", Iw, al) + cross(om, np.einsum("nkij,nkj->nki", Iw, om))
    tau = np.zeros((n, 39))
    for k in range(R.NI):
        J = JR.jac_at(c, [R.INERT_MV[k]], pc[:, k:k + 1], vel_at_com)[:, 0]
        tau += np.einsum("nic,ni->nc", J[:, 0:3], f[:, k]) + np.einsum("nic,ni->nc", J[:, 3:6], nk[:, k])
    tau[:, 6:] += arm.astype(np.float64) * acc[:, 6:]
    worst = float(np.abs(tau - ref["tau"]).max())
    # and the bias forces: the same advance with a = 0
    zero = np.zeros_like(acc)
    (vp, wp), (vm, wm) = (com_velocities(R.chain(*advanced(root, dof, zero, pr, s, h), np.float64, vel_at_com)) for s in (1.0, -1.0))
    cdd, al = (vp - vm) / (2 * h), (wp - wm) / (2 * h)
    f = w[..., None] * (cdd - G64)
    nk = np.einsum("nkij,nkj->nki", Iw, al) + cross(om, np.einsum("nkij,nkj->nki", Iw, om))
    bias = np.zeros((n, 39))
    for k in range(R.NI):
        J = JR.jac_at(c, [R.INERT_MV[k]], pc[:, k:k + 1], vel_at_com)[:, 0]
        bias += np.einsum("nic,ni->nc", J[:, 0:3], f[:, k]) + np.einsum("nic,ni->nc", J[:, 3:6], nk[:, k])
    worst_b = float(np.abs(bias - ref["bias"]).max())
    print("central differences of the chain's velocities: tau %.2e, bias %.2e on values up to %.0f" % (worst, worst_b, np.abs(ref["tau"]).max()))
    assert worst < 1e-4 and worst_b < 1e-4


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_reference_power_balance(vel_at_com):
    """Without gravity the bias forces' power is the rate of the kinetic energy that M's change alone causes: nu . h == nu' Mdot nu / 2, Mdot by
    central differences, h = 1e-6, of jacobians_ref.mass_matrix along the same advance.  The allowance is the differences' rounding, 4 ulp of
    the largest entry of M over h per entry of Mdot, through |nu|' . |nu| / 2 (truncation, h^2 / 6 times a third derivative of M, is a
    thousandth of it)."""
    h, n = 1e-6, 16
    root, dof, ms, _arm, _acc = DR.seeded(n, 81)
    root, dof = root.astype(np.float64), dof.astype(np.float64)
    c = R.chain(root, dof, np.float64, vel_at_com)
    hb = DR.evaluate(root, dof, vel_at_com, ms, g=(0.0, 0.0, 0.0), c=c)
    assert np.abs(hb["gravity"]).max() == 0.0
    pr = JR.p_ref(c, vel_at_com)
    zero = np.zeros((n, 39))
    Mp, Mm = (JR.mass_matrix(R.chain(*advanced(root, dof, zero, pr, s, h), np.float64, vel_at_com), vel_at_com, ms)[0] for s in (1.0, -1.0))
    nu = JR.nu(root, dof)
    lhs = (nu * (hb["bias"] - hb["gravity"])).sum(-1)
    rhs = 0.5 * np.einsum("na,nab,nb->n", nu, (Mp - Mm) / (2 * h), nu)
    allow = 0.5 * np.abs(nu).sum(-1) ** 2 * 4 * 2.0 ** -52 * np.abs(Mp).max(axis=(1, 2)) / h
    print("power balance: %.2e W off on up to %.0f W, %.3f of the allowance" % (np.abs(lhs - rhs).max(), np.abs(rhs).max(), (np.abs(lhs - rhs) / allow).max()))
    assert (np.abs(lhs - rhs) <= allow).all()


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_reference_gravity_and_momentum_against_the_centre_of_mass(ref8, vel_at_com):
    r = ref8[vel_at_com]
    c, out = r["c"], r["out"]
    co, cv, mass = R.com(c, ref8["ms"])
    pr = JR.p_ref(c, vel_at_com)
    wg = mass[:, None] * G64
    e1 = np.abs(out["gravity"][:, 0:3] + wg).max()
    e2 = np.abs(out["gravity"][:, 3:6] + cross(co - pr, wg)).max()
    e3 = np.abs(out["momentum"][:, 0:3] - mass[:, None] * cv).max()
    # the angular momentum shifted to p_ref is the angular rows of M nu (M without the armature: rows 0:6 hold none)
    nu = JR.nu(ref8["root"], ref8["dof"])
    Lp = out["momentum"][:, 3:6] + cross(co - pr, out["momentum"][:, 0:3])
    e4 = np.abs(Lp - np.einsum("nab,nb->na", r["M"], nu)[:, 3:6]).max()
    e5 = np.abs(out["momentum"][:, 0:3] - np.einsum("nab,nb->na", r["M"], nu)[:, 0:3]).max()
    print("gravity force %.1e N, gravity moment %.1e N m, momentum %.1e, about p_ref against M nu %.1e, linear against M nu %.1e" % (e1, e2, e3, e4, e5))
    assert max(e1, e2, e3, e4, e5) < 1e-11
    # the rate of linear momentum the velocities alone cause: bias - gravity, rows 0:3, is sum_k w_k cdd_k at nu_dot = 0
    kin = DR.kinematics(c, ref8["dof"], vel_at_com)
    f, _n = DR.wrenches(c, kin, JR.records(c, ref8["ms"]), np.zeros(3))
    assert np.abs(out["bias"][:, 0:3] - out["gravity"][:, 0:3] - f.sum(1)).max() < 1e-10


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_reference_momentum_against_the_dense_dynamics(ref8, vel_at_com):
    """tests/dense_dynamics_np.py's spatial momentum is taken about the world origin: shifted to the centre of mass it is ours."""
    from dense_dynamics_np import DenseDynamics, body_twist_from_root
    model = load_model()
    dd = DenseDynamics(model)
    root, dof, ms = ref8["root"], ref8["dof"], ref8["ms"].astype(np.float64)
    co, _cv, _m = R.com(ref8[vel_at_com]["c"], ref8["ms"])
    worst = 0.0
    for e in range(8):
        nu_b = body_twist_from_root(root[e], model.inert_com[R.RECORD[0]], bool(vel_at_com))
        _ke, _pe, mom = dd.energy_momentum(root[e, 0:3], root[e, 3:7], dof[e, :, 0], nu_b, dof[e, :, 1], ms[e], np.zeros(33), G64)
        L = mom[0:3] - np.cross(root[e, 0:3] + co[e], mom[3:6])
        worst = max(worst, float(np.abs(np.concatenate([mom[3:6], L]) - ref8[vel_at_com]["out"]["momentum"][e]).max()))
    print("momentum against the dense dynamics: %.2e" % worst)
    assert worst < 1e-11


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_reference_against_the_dense_forward_dynamics(ref8, vel_at_com):
    """DenseDynamics.accelerations with zero damping, dt = 0 and seeded joint torques gives the derivative of [w_b, v_b, qd] (the base twist
    in base coordinates, v_b the base ORIGIN's velocity).  In our coordinates: alpha = R wdot_b; the origin's classical acceleration
    R vdot_b + omega x R v_b (the spatial linear acceleration at the world origin, plus alpha x p + omega x v_origin, is the same number); then
    to p_ref: + alpha x p_ref + omega x (omega x p_ref).  Then M a + h == [0; tau], to the rounding of the 39-term rows and of the solve."""
    from dense_dynamics_np import DenseDynamics, body_twist_from_root
    model = load_model()
    dd = DenseDynamics(model)
    root, dof, ms, arm = ref8["root"], ref8["dof"], ref8["ms"].astype(np.float64), ref8["arm"].astype(np.float64)
    tau = np.random.default_rng(91).normal(0, 50, (8, 33))
    acc = np.zeros((8, 39))
    pr = JR.p_ref(ref8[vel_at_com]["c"], vel_at_com)
    for e in range(8):
        nu_b = body_twist_from_root(root[e], model.inert_com[R.RECORD[0]], bool(vel_at_com))
        ab, qdd, t = dd.accelerations(root[e, 0:3], root[e, 3:7], dof[e, :, 0], nu_b, dof[e, :, 1], ms[e], arm[e], np.zeros(33), 0.0, G64, tau[e])
        R0 = t["Rw"][0]
        om, al = R0 @ nu_b[0:3], R0 @ ab[0:3]
        xdd = R0 @ ab[3:6] + np.cross(om, R0 @ nu_b[3:6])
        acc[e, 0:3] = xdd + np.cross(al, pr[e]) + np.cross(om, np.cross(om, pr[e]))
        acc[e, 3:6], acc[e, 6:] = al, qdd
    got = DR.evaluate(root, dof, vel_at_com, ref8["ms"], ref8["arm"], acc, c=ref8[vel_at_com]["c"])["tau"]
    want = np.concatenate([np.zeros((8, 6)), tau], 1)
    # the rows' own rounding, entry by entry, plus the solve's residual, which is bounded by norms only: 3 n ulp |M|_inf |a|_inf for Gaussian
    # elimination with a growth factor of order one (n = 39)
    M = ref8[vel_at_com]["M"]
    allow = 256 * 2.0 ** -52 * (np.einsum("nab,nb->na", np.abs(M), np.abs(acc)) + np.abs(ref8[vel_at_com]["out"]["bias"]) + np.abs(want))
    allow = allow + (3 * 39 * 2.0 ** -52 * np.abs(M).sum(-1).max(-1) * np.abs(acc).max(-1))[:, None]
    err = np.abs(got - want)
    print("M a + h against [0; tau] of the dense forward dynamics: %.2e with |a| up to %.0f, %.3f of the allowance" % (err.max(), np.abs(acc).max(), (err / allow).max()))
    assert (err <= allow).all()


# ---------------------------------------------------------------------------------------------- 2. the g++ build against float64
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/dynamics_host.cpp")
    so = str(tmp_path_factory.mktemp("dwnh") / "libdwnh.so")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, os.path.join(ROOT, "tests", "dynamics_host.cpp")])
    lib = C.CDLL(so)
    lib.dwnh_inverse_dynamics.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_float] * 3 + [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    lib.dwnh_pack_table.argtypes = [C.POINTER(JM.DwjModel), C.c_void_p, C.c_char_p, C.c_int]
    table, err = np.zeros(DM.TABLE_WORDS, U), C.create_string_buffer(256)
    m = JM.model_struct(load_model())
    assert lib.dwnh_pack_table(C.byref(m), _p(table), err, 256) == 0, err.value
    lib.table = table
    return lib


def host_run(lib, root, dof, ms, arm, acc, vel_at_com, outs=OUTS, g=DR.GRAVITY, into=None):
    """The outputs named, NaN-filled beforehand, as a dict (the others None)."""
    n = len(root)
    o = {k: np.full((n, 6 if k == "momentum" else 39), np.nan, F) if k in outs else None for k in OUTS} if into is None else into
    rc = lib.dwnh_inverse_dynamics(n, _p(lib.table), _p(root), _p(dof), _p(ms), _p(arm), g[0], g[1], g[2], _p(acc), vel_at_com,
                                   _p(o["bias"]), _p(o["gravity"]), _p(o["tau"]), _p(o["momentum"]))
    assert rc == 0
    return o


def same(a, b):
    """Number for number: equal as floats (a zero's sign apart), NaN nowhere."""
    return bool(np.isfinite(a).all() and np.isfinite(b).all() and (a == b).all())


def test_the_library_and_the_host_build_pack_the_same_table(host):
    api = cbind.declare(C.CDLL(build.build()), "dyros_dynamics.h", "dwn_")
    japi = cbind.declare(C.CDLL(build.build()), "dyros_jacobians.h", "dwj_")
    t = DM.pack_table(api, load_model())
    assert t.dtype == U and t.shape == (DM.TABLE_WORDS,) and np.array_equal(t, host.table) and np.array_equal(t, JM.pack_table(japi, load_model()))
    # it refuses what dwj_pack_table refuses, under its own name
    d = {k: np.array(v) for k, v in load_model().d.items() if k in ("mv_parent", "mv_pos", "mv_rot0", "mv_axis", "body_moving", "inert_gym", "inert_mv", "inert_mass",
                                                                     "inert_com", "inert_I")}
    d["mv_parent"][5] = 6
    with pytest.raises(cbind.DyrosWalkLibraryError, match="dwn_pack_table: a child precedes its parent"):
        DM.pack_table(api, d)
    d["mv_parent"][5] = load_model().d["mv_parent"][5]
    d["inert_I"][9][1][1] = float("nan")
    with pytest.raises(cbind.DyrosWalkLibraryError, match="dwn_pack_table: inert_I is not finite"):
        DM.pack_table(api, d)


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_host_build_against_float64(host, vel_at_com):
    root, dof, ms, arm, acc = DR.seeded(N, 11 + vel_at_com)
    o = host_run(host, root, dof, ms, arm, acc, vel_at_com)
    ex = DR.excess(o, root, dof, ms, arm, acc, vel_at_com, report="host N=%d vel_at_com=%d" % (N, vel_at_com))
    assert len(ex) == len(DR.CHANNELS) and DR.within(ex), ex
    # nominal masses, no armature, another gravity vector
    g = (1.5, -2.0, -3.71)
    o = host_run(host, root, dof, None, None, acc, vel_at_com, g=g)
    ex = DR.excess(o, root, dof, None, None, acc, vel_at_com, g=g, report="host, nominal masses, no armature, g = %s" % (g,))
    assert DR.within(ex), ex


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_exact_properties(host, vel_at_com):
    root, dof, ms, arm, acc = DR.seeded(N, 21)
    o = host_run(host, root, dof, ms, arm, acc, vel_at_com)
    assert all(np.isfinite(o[k]).all() for k in OUTS)
    # 640 m out: the same bits
    far = root.copy()
    far[:, 0:2] += np.array([640.0, -640.0], F)
    of = host_run(host, far, dof, ms, arm, acc, vel_at_com)
    assert all(np.array_equal(of[k].view(U), o[k].view(U)) for k in OUTS)
    # every velocity zeroed: bias is gravity, and the momentum is zero
    still_r, still_d = root.copy(), dof.copy()
    still_r[:, 7:13], still_d[:, :, 1] = 0, 0
    os_ = host_run(host, still_r, still_d, ms, arm, acc, vel_at_com)
    assert same(os_["bias"], os_["gravity"]) and same(os_["gravity"], o["gravity"]) and (os_["momentum"] == 0).all()
    # accel = 0: tau is bias
    oz = host_run(host, root, dof, ms, arm, np.zeros_like(acc), vel_at_com)
    assert same(oz["tau"], oz["bias"]) and np.array_equal(oz["bias"].view(U), o["bias"].view(U))
    # the armature is added last, on the joints only; without tau it does not enter
    on = host_run(host, root, dof, ms, None, acc, vel_at_com)
    assert np.array_equal(on["tau"][:, :6].view(U), o["tau"][:, :6].view(U)) and np.array_equal((on["tau"][:, 6:] + arm * acc[:, 6:]).view(U), o["tau"][:, 6:].view(U))
    assert all(np.array_equal(on[k].view(U), o[k].view(U)) for k in ("bias", "gravity", "momentum"))
    # gravity's force is the weight: -g times the total mass, whatever the pose, and g = 0 gives exactly nothing
    o0 = host_run(host, root, dof, ms, arm, acc, vel_at_com, g=(0.0, 0.0, 0.0))
    assert (o0["gravity"] == 0).all() and np.array_equal(o0["momentum"].view(U), o["momentum"].view(U))
    assert (o["gravity"][:, 0:2] == 0).all() and (o["gravity"][:, 2] > 0).all()


def test_a_null_output_leaves_the_others_bits(host):
    root, dof, ms, arm, acc = DR.seeded(N, 31)
    full = host_run(host, root, dof, ms, arm, acc, 1)
    for k in OUTS:
        one = host_run(host, root, dof, ms, arm, acc, 1, outs=(k,))
        assert np.array_equal(one[k].view(U), full[k].view(U)) and all(one[j] is None for j in OUTS if j != k), k
        rest = host_run(host, root, dof, ms, arm, acc, 1, outs=tuple(j for j in OUTS if j != k))
        assert all(np.array_equal(rest[j].view(U), full[j].view(U)) for j in OUTS if j != k), k
    # without accel: bias, gravity and momentum are what they were
    o = host_run(host, root, dof, ms, arm, None, 1, outs=("bias", "gravity", "momentum"))
    assert all(np.array_equal(o[j].view(U), full[j].view(U)) for j in ("bias", "gravity", "momentum"))


def test_non_finite_inputs_stay_in_their_env(host):
    root, dof, ms, arm, acc = DR.seeded(6, 41)
    o0 = host_run(host, root, dof, ms, arm, acc, 1)
    root[2, 4], dof[3, 20, 0], acc[5, 7] = np.nan, np.inf, np.nan
    o = host_run(host, root, dof, ms, arm, acc, 1)
    for k in OUTS:
        assert np.array_equal(o[k][[0, 1, 4]].view(U), o0[k][[0, 1, 4]].view(U)), k
        assert np.isnan(o[k][2]).any() and np.isnan(o[k][3]).any(), k
    # a NaN in accel reaches tau alone
    assert np.isnan(o["tau"][5]).any() and all(np.array_equal(o[k][5].view(U), o0[k][5].view(U)) for k in ("bias", "gravity", "momentum"))


# ---------------------------------------------------------------------------------------------- 3. the ABI
@pytest.fixture(scope="module")
def api():
    return cbind.declare(C.CDLL(build.build()), "dyros_dynamics.h", "dwn_")


@pytest.mark.parametrize("check", ["prototypes", "layouts"])
def test_header_python_and_library_agree(check, tmp_path):
    import test_cbind as TC
    if check == "prototypes":
        TC.test_ctypes_prototypes_match_the_header("dyros_dynamics.h", "dwn_", "dynamics", C.CDLL(build.build()))
    else:
        TC.test_struct_layouts_match_the_host_compiler("dyros_dynamics.h", "dwn_", "dynamics", tmp_path)          # (it declares no struct of its own)
    assert sorted(DM.EXPORTS) == ["abi_version", "inverse_dynamics", "last_error", "pack_table"]
    assert dict(build.SOURCES)[SRC] == ["-ffp-contract=off"] and "dw_dynamics.h" in build.HEADERS
    K, KJ = DM.K, JM.K
    assert K["DWN_ABI_VERSION"] == 1 and (K["DWN_NV"], K["DWN_MOM"]) == (39, 6)
    for name in ("NUM_BODIES", "NUM_MOVING", "NUM_DOF", "NUM_INERT", "NV", "TABLE_WORDS"):
        assert K["DWN_" + name] == KJ["DWJ_" + name]
    assert K["DWN_GROUP"] * K["DWN_LANES"] == 256 and K["DWN_GROUP"] * 36 <= 256
    assert DM.DEFAULTS == {"bias": True, "gravity": True, "inverse_dynamics": False, "momentum": False, "armature": True, "auto": False}
    # the header says what bias does not hold
    text = open(os.path.join(ROOT, "include", "dyros_dynamics.h")).read()
    assert "NO joint damping, NO friction and NO actuator" in text
    # the older headers are untouched
    assert KJ["DWJ_ABI_VERSION"] == 1 and cbind.constants("dyros_bodies.h", "dwb_")["DWB_ABI_VERSION"] == 1


def test_refusals_happen_before_any_launch(api):
    """Every buffer is NULL or a host address here: a launch would fault, a refusal returns -1 with its message."""
    one = C.c_void_p(16)
    g = (0.0, 0.0, -9.81)
    ok = lambda **kw: tuple(dict(dict(n=8, table=one, root=one, dof=one, ms=None, arm=None, gx=g[0], gy=g[1], gz=g[2], acc=None, vac=0, bias=one,          # noqa: E731
                                      gravity=None, tau=None, mom=None, stream=None), **kw).values())
    for args, msg in ((ok(n=0), b"num_envs"), (ok(n=-3), b"num_envs"), (ok(n=1 << 30), b"num_envs"),
                      (ok(table=None), b"a buffer is missing"), (ok(root=None), b"a buffer is missing"), (ok(dof=None), b"a buffer is missing"),
                      (ok(table=C.c_void_p(8)), b"16-byte aligned"),
                      (ok(tau=one), b"tau needs accel"), (ok(bias=None, tau=one), b"tau needs accel"),
                      (ok(bias=None), b"no output"), (ok(bias=None, acc=one), b"no output"),
                      (ok(gz=float("nan")), b"not finite"), (ok(gx=float("inf")), b"not finite"), (ok(gy=float("-inf"), mom=one), b"not finite")):
        assert api["inverse_dynamics"](*args) == -1 and msg in api["last_error"]() and b"dwn_inverse_dynamics" in api["last_error"](), (args, api["last_error"]())


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
    assert "dwn_k_inverse_dynamics" in names[0]
    for n, s, l in zip(names, scratch, lds):
        assert "dwn_k_" in n and s == 0 and l <= 65536, (n, s, l)
        assert not any(x in n for x in tuple(TAKEN) + tuple(TAKEN_BODIES) + ("dwg_k_", "dwb_k_", "dwf_k_", "dwj_k_")), n
    print("dwn_k_inverse_dynamics: LDS %d bytes per workgroup" % lds[0])


# ---------------------------------------------------------------------------------------------- 5. the Python surface
def test_cfg_spec():
    full = {"bias": True, "gravity": True, "inverse_dynamics": False, "momentum": False, "armature": True, "auto": False}
    assert DM.resolve(None) is None and DM.resolve(False) is None
    assert DM.resolve(True) == DM.resolve({}) == full
    s = DM.resolve({"bias": False, "inverse_dynamics": True, "momentum": True, "auto": True, "armature": False})
    assert s == {"bias": False, "gravity": True, "inverse_dynamics": True, "momentum": True, "armature": False, "auto": True}
    assert DM.resolve({"bias": False, "gravity": False, "momentum": True})["momentum"] is True
    for bad in (1, "on", ["bias"], {"h": True}, {"bias": 1}, {"gravity": None}, {"inverse_dynamics": "yes"}, {"momentum": 0}, {"armature": 1.0}, {"auto": "no"},
                {"bias": False, "gravity": False}, {"bias": False, "gravity": False, "auto": True, "armature": True}, {1: True}):
        with pytest.raises(ValueError):
            DM.resolve(bad)
    with pytest.raises(ValueError, match="nothing to compute"):
        DM.resolve({"bias": False, "gravity": False})
    from isaacgymdyros_amd.config import default_cfg, validate_cfg
    cfg = default_cfg(64, "cpu")
    assert "dynamics" not in cfg["sim"]["mi355"] and "amp_dynamics" not in cfg["sim"]["mi355"]          # (off by default)
    for key in ("dynamics", "amp_dynamics"):
        cfg = default_cfg(64, "cpu")
        cfg["sim"]["mi355"][key] = {"inverse_dynamics": True, "momentum": True, "auto": True}
        validate_cfg(cfg)
        cfg["sim"]["mi355"][key] = True
        validate_cfg(cfg)
        for bad in ({"mass": True}, {"bias": 1}, {"bias": False, "gravity": False}, "on"):
            cfg["sim"]["mi355"][key] = bad
            with pytest.raises(ValueError):
                validate_cfg(cfg)
