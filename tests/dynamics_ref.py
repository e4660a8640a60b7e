"""The bias-force, gravity, inverse-dynamics and momentum tensors restated in numpy from the rules of include/dyros_dynamics.h (DESIGN.md
section 24), on top of tests/body_states_ref.py's chain and tests/jacobians_ref.py's dense Jacobians and records; shared by
tests/test_dynamics.py (the g++ build of csrc/dw_dynamics.h) and tests/test_dynamics_gpu.py (the HIP kernel).  Test helper.

The restatement is the header's DEFINITION: classical accelerations by the recursion, then tau = sum_k J_k,lin' f_k + J_k,ang' n_k over 36 dense
[6, 39] Jacobians at the records' COMs -- not the subtree sums about each body's origin that the kernel runs, so agreement is a check of the
algorithm as well.  Float64 is the reference; float32 (the model constants rounded as the device table rounds them) measures what the format
costs.

The tolerance is measured here, against the reference and never against a kernel (tests/body_states_ref.py's method): per channel, d = the
largest deviation of the float32 restatement from the float64 one over STATES seeded states(..., mass=True) with seeded armatures and seeded
nu_dot, and what is tested must be within FACTOR * d.  Channels: base-linear, base-angular and joint words of bias, gravity and tau, and the
linear and angular momentum.  The seeded nu_dot is normal with standard deviation ACCEL_SCALE = (10 m/s^2, 20 rad/s^2, 50 rad/s^2) for the
base's linear, the base's angular and the joints' words: a walking humanoid's joints change a 4 rad/s rate within a tenth of a second.
"""
import functools

import numpy as np

import body_states_ref as R
import jacobians_ref as JR

NB, NM, NI, NV = R.NB, R.NM, R.NI, 39
FACTOR, STATES = R.FACTOR, R.STATES
F = np.float32
GRAVITY = (0.0, 0.0, -9.81)
ACCEL_SCALE = (10.0, 20.0, 50.0)
cross = R.cross


def accel_of(n, seed):
    """Seeded nu_dot [n, 39] float32."""
    r = np.random.default_rng(seed)
    return np.concatenate([r.normal(0, ACCEL_SCALE[0], (n, 3)), r.normal(0, ACCEL_SCALE[1], (n, 3)), r.normal(0, ACCEL_SCALE[2], (n, 33))], 1).astype(F)


def gvec(g, dt):
    """The gravity vector as the C call receives it: three float32 scalars."""
    return np.asarray(GRAVITY if g is None else g, F).astype(dt)


def kinematics(c, dof, vel_at_com, a=None, vel=True):
    """(omega, alpha, xdd) [N, 34, 3] each: the angular velocity, angular acceleration and classical origin acceleration that (q, nu, a) imply,
    by the header's recursion.  a None: nu_dot = 0; vel False: nu = 0."""
    dt = c["off"].dtype
    N = len(c["off"])
    qd = np.asarray(dof).astype(dt).reshape(N, 33, 2)[..., 1] if vel else np.zeros((N, 33), dt)
    a = np.zeros((N, NV), dt) if a is None else np.asarray(a).astype(dt)          # (callers hand float32 nu_dot, or float64 in the float64 tests)
    pr, ax = JR.p_ref(c, vel_at_com), JR.axes(c)
    om, al, xdd = np.zeros((N, NM, 3), dt), np.zeros((N, NM, 3), dt), np.zeros((N, NM, 3), dt)
    if vel:
        om[:, 0] = c["w"][:, 0]
    al[:, 0] = a[:, 3:6]
    xdd[:, 0] = a[:, 0:3] - cross(al[:, 0], pr) - cross(om[:, 0], cross(om[:, 0], pr))
    for b in range(1, NM):
        p = R.MV_PARENT[b]
        r = c["off"][:, b] - c["off"][:, p]
        aq = ax[:, b] * qd[:, b - 1, None]
        om[:, b] = om[:, p] + aq
        al[:, b] = al[:, p] + ax[:, b] * a[:, 5 + b, None] + cross(om[:, p], aq)
        xdd[:, b] = xdd[:, p] + cross(al[:, p], r) + cross(om[:, p], cross(om[:, p], r))
    return om, al, xdd


def wrenches(c, kin, rec, g):
    """(f [N, 36, 3], n [N, 36, 3]) of the records: f_k = w_k (cdd_k - g), n_k = Ib_k alpha + omega x (Ib_k omega)."""
    om, al, xdd = (x[:, R.INERT_MV] for x in kin)
    w, pc, Iw = rec
    d = pc - c["off"][:, R.INERT_MV]
    cdd = xdd + cross(al, d) + cross(om, cross(om, d))
    f = w[..., None] * (cdd - g)
    n = np.einsum("nkij,nkj->nki", Iw, al) + cross(om, np.einsum("nkij,nkj->nki", Iw, om))
    return f, n


def momentum_of(c, rec):
    """[N, 6]: sum_k w_k cd_k, then the angular momentum about the centre of mass."""
    w, pc, Iw = rec
    om = c["w"][:, R.INERT_MV]
    cd = c["vo"][:, R.INERT_MV] + cross(om, pc - c["off"][:, R.INERT_MV])
    p = w[..., None] * cd
    com = (w[..., None] * pc).sum(1) / w.sum(1)[:, None]
    L = (cross(pc - com[:, None], p) + np.einsum("nkij,nkj->nki", Iw, om)).sum(1)
    return np.concatenate([p.sum(1), L], 1)


def evaluate(root, dof, vel_at_com, ms=None, arm=None, accel=None, g=None, dtype=np.float64, c=None):
    """dict of bias, gravity [N, 39], tau [N, 39] (when accel is given) and momentum [N, 6] in one number format."""
    c = R.chain(root, dof, dtype, vel_at_com) if c is None else c
    dt = c["off"].dtype
    g = gvec(g, dt)
    rec = JR.records(c, ms)
    pairs = {"bias": wrenches(c, kinematics(c, dof, vel_at_com), rec, g), "gravity": wrenches(c, kinematics(c, dof, vel_at_com, vel=False), rec, g)}
    if accel is not None:
        pairs["tau"] = wrenches(c, kinematics(c, dof, vel_at_com, accel), rec, g)
    out = {k: np.zeros((len(c["off"]), NV), dt) for k in pairs}
    ax = JR.axes(c)
    for k in range(NI):
        J = JR.jac_at(c, [R.INERT_MV[k]], rec[1][:, k:k + 1], vel_at_com, ax)[:, 0]
        for name, (f, n) in pairs.items():
            out[name] += np.einsum("nic,ni->nc", J[:, 0:3], f[:, k]) + np.einsum("nic,ni->nc", J[:, 3:6], n[:, k])
    if accel is not None and arm is not None:
        out["tau"][:, 6:] += np.asarray(arm, F).astype(dt) * np.asarray(accel).astype(dt)[:, 6:]
    out["momentum"] = momentum_of(c, rec)
    return out


# ---------------------------------------------------------------------------------------------- the tolerance
CHANNELS = tuple("%s_%s" % (t, p) for t in ("bias", "gravity", "tau") for p in ("lin", "ang", "joint")) + ("momentum_lin", "momentum_ang")


def split(out):
    """The channels of a dict of outputs (any subset) as a dict of arrays."""
    ch = {}
    for t in ("bias", "gravity", "tau"):
        if out.get(t) is not None:
            ch[t + "_lin"], ch[t + "_ang"], ch[t + "_joint"] = out[t][..., 0:3], out[t][..., 3:6], out[t][..., 6:]
    if out.get("momentum") is not None:
        ch["momentum_lin"], ch["momentum_ang"] = out["momentum"][..., 0:3], out["momentum"][..., 3:6]
    return ch


def seeded(n, seed):
    """Seeded inputs for n envs: (root, dof, mass_scale, armature, accel), float32."""
    root, dof, ms = R.states(n, seed, mass=True)
    return root, dof, ms, JR.armature_of(n, seed + 1), accel_of(n, seed + 2)


@functools.lru_cache(maxsize=None)
def measured(vel_at_com):
    """d per channel: the float32 restatement against the float64 one at STATES seeded states."""
    root, dof, ms, arm, acc = seeded(STATES, 24000 + 10 * vel_at_com)
    a, b = (split(evaluate(root, dof, vel_at_com, ms, arm, acc, dtype=dt)) for dt in (np.float64, np.float32))
    return {ch: float(np.abs(a[ch] - b[ch].astype(np.float64)).max()) for ch in CHANNELS}


def excess(got, root, dof, ms, arm, accel, vel_at_com, g=None, report=None, want=None):
    """Every channel of the outputs in dict `got` (bias, gravity, tau, momentum; any subset) against the float64 reference, as the largest
    deviation divided by FACTOR * d: a dict channel -> ratio; all must be <= 1."""
    d = measured(int(bool(vel_at_com)))
    want = split(evaluate(root, dof, vel_at_com, ms, arm, accel, g) if want is None else want)
    have = split({k: None if v is None else np.asarray(v, F).astype(np.float64) for k, v in got.items()})
    out = {ch: float(np.abs(have[ch] - want[ch]).max() / (FACTOR * d[ch])) for ch in have}
    if report is not None:
        print(report, {k: round(v, 3) for k, v in out.items()}, "d:", {k: "%.2e" % v for k, v in d.items()})
    return out


def within(ex: dict) -> bool:
    return len(ex) > 0 and all(np.isfinite(v) and v <= 1.0 for v in ex.values())
