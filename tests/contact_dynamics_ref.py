"""The contact-consistent dynamics restated in numpy from the rules of include/dyros_contact_dynamics.h, on top of
tests/body_states_ref.py's chain, tests/jacobians_ref.py's dense Jacobians (jac_at), tests/dynamics_ref.py's recursion (kinematics) and
tests/forward_dynamics_ref.py's mass matrix and pattern arithmetic; shared by tests/test_contact_dynamics.py (the g++ build of
csrc/dw_contact.h) and tests/test_contact_dynamics_gpu.py (the HIP kernel).  Test helper.

The reference is float64 and does NOT take the Schur path: accel and force come from np.linalg.solve of the dense (39 + m)-square KKT matrix
[[M, -J_c'], [J_c, 0]], minv_jt from np.linalg.solve of M, lambda_inv as J_c M^-1 J_c' and lambda as np.linalg.inv of it.

The tolerance is measured here, against the reference and never against a kernel (tests/body_states_ref.py's method): per channel, d = the
largest deviation of the float32 run of the whole pipeline (the chain, M, the LTDL on the pattern, the sweeps, A, its dense L D L', the small
sweeps, the combination) from the float64 reference over STATES seeded states (dynamics_ref.seeded), for each velocity mode and each contact
set (K = 1, 2 and 4), and what is tested must be within FACTOR * d.  The right-hand sides are M64 accel_of(...) rounded to float32 minus the
float32 bias forces, so that b has the size of real generalised forces.  The solve is linear in (b, gamma - Jd_c nu), so accel's and force's
allowances grow with the solution, as forward_dynamics_ref.x_allowance's does: an env and right-hand side whose largest accel (force) word
is s times the largest d was measured with gets s d.
"""
import functools

import numpy as np

import body_states_ref as R
import dynamics_ref as DR
import forward_dynamics_ref as FR
import jacobians_ref as JR

NV, NM = 39, R.NM
FACTOR, STATES = R.FACTOR, R.STATES
F = np.float32
NAMES = list(R.MODEL.body_names)
FEET = (("L_Foot_Link", (0.0, 0.0, -0.09)), ("R_Foot_Link", (0.0, 0.0, -0.09)))
# the contact sets of the tests: one foot, both feet (the default), feet and both wrists (points off the bodies' origins)
SETS = {1: FEET[:1], 2: FEET, 4: FEET + (("L_Wrist2_Link", (0.02, -0.01, -0.05)), ("R_Wrist2_Link", (0.02, 0.01, -0.05)))}
CHANNELS = ("jc_lin", "jc_ang", "jdnu_lin", "jdnu_ang", "minv_jt", "lambda_inv", "lambda", "accel_lin", "accel_ang", "accel_joint", "force_f", "force_n")
OUTS = ("jc", "jdnu", "minv_jt", "lambda_inv", "lambda", "accel", "force")


def ids_of(contacts):
    return [NAMES.index(b) if isinstance(b, str) else int(b) for b, _ in contacts]


def carriers(contacts):
    return [R.CARRIER[g] for g in ids_of(contacts)]


def arms(c, contacts):
    """r = R_b pos [N, K, 3] of the contacts' points."""
    dt = c["off"].dtype
    return np.stack([R.mv3(c["R"][:, b], np.asarray(pos, F).astype(dt)) for b, (_, pos) in zip(carriers(contacts), contacts)], 1)


def jc_of(c, contacts, vel_at_com):
    """J_c [N, 6 K, 39]."""
    m = carriers(contacts)
    return JR.jac_at(c, m, c["off"][:, m] + arms(c, contacts), vel_at_com).reshape(len(c["off"]), 6 * len(m), NV)


def jdnu_of(c, dof, contacts, vel_at_com):
    """Jd_c nu [N, 6 K]: the points' classical accelerations and the bodies' angular accelerations at nu_dot = 0."""
    om, al, xdd = (x[:, carriers(contacts)] for x in DR.kinematics(c, dof, vel_at_com))
    r = arms(c, contacts)
    return np.concatenate([xdd + R.cross(al, r) + R.cross(om, R.cross(om, r)), al], -1).reshape(len(r), -1)


def rhs_b(rhs, sub, dtype):
    b = np.asarray(rhs, F).astype(dtype)
    return b if sub is None else b - np.asarray(sub, F).astype(dtype)[:, None, :]


def mirror(X):
    """Rows >= columns of X [N, m, m], mirrored."""
    lower = np.tril(X)
    return lower + np.swapaxes(np.tril(lower, -1), 1, 2)


def front(root, dof, vel_at_com, ms, arm, dtype):
    """(chain, M, L, D) in one number format: what does not depend on the contacts."""
    c = R.chain(root, dof, dtype, vel_at_com)
    M = JR.mass_matrix(c, vel_at_com, ms, arm)[0]
    return (c, M) + FR.ltdl(M)


def evaluate(root, dof, vel_at_com, ms, arm, contacts, rhs=None, sub=None, gamma=None, pre=None):
    """The float64 reference: dict of jc, jdnu, minv_jt, lambda_inv, lambda, M and, when rhs [N, R, 39] is given, accel and force by the dense
    KKT solve.  pre: front(..., np.float64) of the same state."""
    c, M = (pre if pre is not None else front(root, dof, vel_at_com, ms, arm, np.float64))[:2]
    J, jd = jc_of(c, contacts, vel_at_com), jdnu_of(c, dof, contacts, vel_at_com)
    N, m = J.shape[0], J.shape[1]
    Yt = np.linalg.solve(M, np.swapaxes(J, 1, 2))          # [N, 39, m]
    A = J @ Yt
    out = {"jc": J, "jdnu": jd, "minv_jt": np.swapaxes(Yt, 1, 2), "lambda_inv": A, "lambda": np.linalg.inv(A), "M": M}
    if rhs is not None:
        b = rhs_b(rhs, sub, np.float64)
        g = (np.zeros((N, m)) if gamma is None else np.asarray(gamma, F).astype(np.float64)) - jd
        KKT = np.zeros((N, NV + m, NV + m))
        KKT[:, :NV, :NV], KKT[:, :NV, NV:], KKT[:, NV:, :NV] = M, -np.swapaxes(J, 1, 2), J
        right = np.concatenate([b, np.broadcast_to(g[:, None, :], (N, b.shape[1], m))], -1)
        sol = np.swapaxes(np.linalg.solve(KKT, np.swapaxes(right, 1, 2)), 1, 2)
        out["accel"], out["force"], out["KKT"], out["right"] = sol[..., :NV], sol[..., NV:], KKT, right
    return out


def ldl(A):
    """(L [N, m, m] unit lower triangular, D [N, m]) with A = L D L', in A's number format, by the kernel's right-looking updates."""
    H = np.array(A, copy=True)
    m = H.shape[1]
    for j in range(m - 1):
        for i in range(j + 1, m):
            a = H[:, i, j] / H[:, j, j]
            for k in range(j + 1, i + 1):
                H[:, i, k] = H[:, i, k] - a * H[:, k, j]
    D = H[:, np.arange(m), np.arange(m)].copy()
    L = np.tril(H, -1) / D[:, None, :]
    L[:, np.arange(m), np.arange(m)] = 1
    return L.astype(A.dtype), D


def small_solve(L, D, g):
    """A^-1 g for g [N, C, m] by the forward sweep, the division and the backward sweep, in L's number format."""
    g = np.array(g, dtype=L.dtype, copy=True)
    m = g.shape[-1]
    for j in range(m - 1):
        for i in range(j + 1, m):
            g[:, :, i] = g[:, :, i] - L[:, i, j, None] * g[:, :, j]
    g = g / D[:, None, :]
    for j in range(m - 1, 0, -1):
        for i in range(j):
            g[:, :, i] = g[:, :, i] - L[:, j, i, None] * g[:, :, j]
    return g


def dot_rows(J, v):
    """J [N, m, 39] times v [N, C, 39] -> [N, C, m], a column at a time in the operands' number format."""
    out = np.zeros(v.shape[:2] + (J.shape[1],), J.dtype)
    for k in range(NV):
        out = out + J[:, None, :, k] * v[:, :, None, k]
    return out


def schur(root, dof, vel_at_com, ms, arm, contacts, rhs=None, sub=None, gamma=None, dtype=np.float32, pre=None):
    """The same dict by the header's solve, the way the kernel runs it, in one number format: the chain, M, the LTDL on the pattern, the sweeps
    over J_c's rows, A = J_c Y, its dense L D L', x0, A f = (gamma - Jd_c nu) - J_c x0, nu_dot = x0 + Y f."""
    c, M, L, D = pre if pre is not None else front(root, dof, vel_at_com, ms, arm, dtype)
    J, jd = jc_of(c, contacts, vel_at_com), jdnu_of(c, dof, contacts, vel_at_com)
    N, m = J.shape[0], J.shape[1]
    Y = FR.solve(L, D, J)
    A = mirror(np.swapaxes(dot_rows(J, Y), 1, 2))          # [N, r, c] = J[r] . Y[c]
    La, Da = ldl(A)
    out = {"jc": J, "jdnu": jd, "minv_jt": Y, "lambda_inv": A,
           "lambda": mirror(np.swapaxes(small_solve(La, Da, np.broadcast_to(np.eye(m, dtype=dtype), (N, m, m))), 1, 2))}
    if rhs is not None:
        x0 = FR.solve(L, D, rhs_b(rhs, sub, dtype))
        g = ((np.zeros((N, m), dtype) if gamma is None else np.asarray(gamma, F).astype(dtype)) - jd)[:, None, :] - dot_rows(J, x0)
        f = small_solve(La, Da, g)
        acc = x0.copy()
        for i in range(m):
            acc = acc + Y[:, None, i, :] * f[:, :, i, None]
        out["accel"], out["force"] = acc, f
    return out


def rhs_of(root, dof, vel_at_com, ms, arm, nrhs, seed):
    """(rhs [N, nrhs, 39], sub [N, 39]) float32: M64 times seeded accelerations, and the bias forces."""
    return FR.rhs_of(root, dof, vel_at_com, ms, arm, nrhs, seed), DR.evaluate(root, dof, vel_at_com, ms, arm)["bias"].astype(F)


@functools.lru_cache(maxsize=None)
def _measured_state(vel_at_com, plain):
    root, dof, ms, arm, _acc = DR.seeded(STATES, 26000 + 10 * vel_at_com)
    if plain:
        ms = arm = None
    pre = front(root, dof, vel_at_com, ms, arm, np.float64)
    rhs = np.einsum("nab,nrb->nra", pre[1], DR.accel_of(STATES, 26005).astype(np.float64)[:, None]).astype(F)
    sub = DR.evaluate(root, dof, vel_at_com, ms, arm, c=pre[0])["bias"].astype(F)
    return root, dof, ms, arm, rhs, sub, pre, front(root, dof, vel_at_com, ms, arm, np.float32)


def gamma_of(n, m, seed):
    """Seeded commanded accelerations [n, m] float32, dynamics_ref's scales: 10 m/s^2 and 20 rad/s^2."""
    r = np.random.default_rng(seed)
    return (r.normal(0, 1, (n, m // 6, 6)) * np.array([10.0] * 3 + [20.0] * 3)).reshape(n, m).astype(F)


def split(out):
    ch = {}

    def rows(x, axis):          # (linear rows, angular rows) of a tensor whose `axis` runs over the 6 K constraint rows
        x = np.moveaxis(x, axis, -1)
        x = x.reshape(x.shape[:-1] + (-1, 6))
        return x[..., 0:3], x[..., 3:6]
    if out.get("jc") is not None:
        ch["jc_lin"], ch["jc_ang"] = rows(out["jc"], -2)
    if out.get("jdnu") is not None:
        ch["jdnu_lin"], ch["jdnu_ang"] = rows(out["jdnu"], -1)
    for k in ("minv_jt", "lambda_inv", "lambda"):
        if out.get(k) is not None:
            ch[k] = out[k]
    if out.get("accel") is not None:
        ch["accel_lin"], ch["accel_ang"], ch["accel_joint"] = out["accel"][..., 0:3], out["accel"][..., 3:6], out["accel"][..., 6:]
    if out.get("force") is not None:
        ch["force_f"], ch["force_n"] = rows(out["force"], -1)
    return ch


@functools.lru_cache(maxsize=None)
def measured(vel_at_com, K, plain=False):
    """d per channel: the float32 run of the pipeline against the float64 reference at STATES seeded states.  plain: the same states with nominal
    masses and no armature -- another matrix, so it has a d of its own (forward_dynamics_ref.measured)."""
    root, dof, ms, arm, rhs, sub, pre64, pre32 = _measured_state(vel_at_com, plain)
    gamma = gamma_of(STATES, 6 * K, 26007)
    want = evaluate(root, dof, vel_at_com, ms, arm, SETS[K], rhs, sub, gamma, pre=pre64)
    a, b = split(want), split(schur(root, dof, vel_at_com, ms, arm, SETS[K], rhs, sub, gamma, pre=pre32))
    d = {ch: float(np.abs(a[ch] - b[ch].astype(np.float64)).max()) for ch in CHANNELS}
    d["accel_scale"], d["force_scale"] = float(np.abs(want["accel"]).max()), float(np.abs(want["force"]).max())
    d["cond"] = float(np.linalg.cond(want["lambda_inv"]).max())
    return d


def excess(got, root, dof, ms, arm, vel_at_com, K, rhs=None, sub=None, gamma=None, report=None, want=None):
    """Every channel of the outputs in dict `got` (any subset of OUTS) for contact set SETS[K] against the float64 reference, as the largest
    deviation divided by FACTOR * d (accel and force: d scaled with the solution): a dict channel -> ratio; all must be <= 1.  ms and arm both
    None: the d of measured(..., plain=True)."""
    d = measured(int(bool(vel_at_com)), K, ms is None and arm is None)
    full = evaluate(root, dof, vel_at_com, ms, arm, SETS[K], rhs, sub, gamma) if want is None else want
    want = split(full)
    have = split({k: None if v is None else np.asarray(v, F).astype(np.float64) for k, v in got.items() if k in OUTS})
    out = {}
    for ch in have:
        dev = np.abs(have[ch] - want[ch])
        if ch.startswith("accel_") or ch.startswith("force_"):
            kind = ch.split("_")[0]
            s = np.maximum(1.0, np.abs(full[kind]).max(-1) / d[kind + "_scale"])          # [N, R]
            dev = dev.reshape(s.shape + (-1,)) / s[..., None]
        out[ch] = float(dev.max() / (FACTOR * d[ch]))
    if report is not None:
        print(report, {k: round(v, 3) for k, v in out.items()}, "d:", {k: "%.2e" % v for k, v in d.items()})
    return out


def allowance(want_full, vel_at_com, K, kind):
    """FACTOR * d per word of accel [..., 39] or force [..., m] of a float64 reference dict, scaled with the solution."""
    d = measured(int(bool(vel_at_com)), K)
    x = want_full[kind]
    s = np.maximum(1.0, np.abs(x).max(-1, keepdims=True) / d[kind + "_scale"])
    if kind == "accel":
        own = np.array([d["accel_lin"]] * 3 + [d["accel_ang"]] * 3 + [d["accel_joint"]] * 33)
    else:
        own = np.array(([d["force_f"]] * 3 + [d["force_n"]] * 3) * K)
    return FACTOR * own * s


def within(ex: dict) -> bool:
    return len(ex) > 0 and all(np.isfinite(v) and v <= 1.0 for v in ex.values())
