"""The contact inverse dynamics restated in numpy from the rules of include/dyros_contact_inverse_dynamics.h, on top of
tests/body_states_ref.py's chain, tests/dynamics_ref.py's recursion and inverse dynamics (evaluate, kinematics) and
tests/contact_dynamics_ref.py's contact Jacobian (jc_of, jdnu_of); shared by tests/test_contact_inverse_dynamics.py (the g++ build of
csrc/dw_contact_inverse.h) and tests/test_contact_inverse_dynamics_gpu.py (the HIP kernel).  Test helper.

The reference is float64 and does NOT take the normal equations the kernel uses: f - f_ref is the minimum-norm solution that np.linalg.lstsq
gives for the W^-1/2-scaled system  (J_b' W^-1/2) z = r[0:6] - J_b' f_ref,  f = f_ref + W^-1/2 z.  contact_accel comes from
dynamics_ref.kinematics(a) at the contact points, not from J_c a + Jd_c nu.

The tolerance is measured here, against the reference and never against a kernel (tests/body_states_ref.py's method): per channel, d = the
largest deviation of the float32 restatement (dynamics_ref's float32 r, contact_dynamics_ref's float32 J_c, then the header's order: G's 21
words, the L D L' without pivoting, the sweeps, f, tau_joint) from the float64 reference over STATES seeded states, for each velocity mode,
each contact set (K = 1, 2 and 4), each set of weights and with or without f_ref; what is tested must be within FACTOR * d.  force and
tau_joint are linear in (r, f_ref), so their allowances grow with the solution as contact_dynamics_ref.allowance's do: an env whose largest
force (torque) word is s times the largest that d was measured with gets s d.  Channels: force_f, force_n (the wrenches' forces and moments),
tau_joint, ca_lin, ca_ang (contact_accel's linear and angular rows).
"""
import functools

import numpy as np

import body_states_ref as R
import contact_dynamics_ref as CR
import dynamics_ref as DR

NV = 39
FACTOR, STATES = R.FACTOR, R.STATES
F = np.float32
SETS = CR.SETS
BASE = (("base_link", (0.0, 0.0, 0.0)),)
CHANNELS = ("force_f", "force_n", "tau_joint", "ca_lin", "ca_ang")
OUTS = ("tau_joint", "force", "contact_accel", "tau_full")
MOMENTS_10 = (1.0, 1.0, 1.0, 10.0, 10.0, 10.0)


def weights_of(weights, K, dtype=np.float64):
    """[6 K]: None (ones), six numbers (every contact's) or [K][6].  One contact: ones, as dwi_pack_table writes them."""
    if weights is None or K == 1:
        return np.ones(6 * K, dtype)
    w = np.asarray(weights, F)
    return (np.tile(w, K) if w.ndim == 1 and w.size == 6 else w.reshape(6 * K)).astype(dtype)


def fref_of(n, m, seed):
    """Seeded prior wrenches [n, m] float32: forces of 200 N, moments of 20 N m."""
    r = np.random.default_rng(seed)
    return (r.normal(0, 1, (n, m // 6, 6)) * np.array([200.0] * 3 + [20.0] * 3)).reshape(n, m).astype(F)


def contact_accel_of(c, dof, contacts, vel_at_com, a):
    """[N, 6 K]: the points' classical acceleration and the bodies' angular acceleration under (q, nu, a), by dynamics_ref.kinematics."""
    om, al, xdd = (x[:, CR.carriers(contacts)] for x in DR.kinematics(c, dof, vel_at_com, a))
    r = CR.arms(c, contacts)
    return np.concatenate([xdd + R.cross(al, r) + R.cross(om, R.cross(om, r)), al], -1).reshape(len(r), -1)


def front(root, dof, vel_at_com, ms, arm, accel, dtype, g=None):
    """(chain, r [N, 39]) in one number format: what does not depend on the contacts.  accel None: zeros."""
    c = R.chain(root, dof, dtype, vel_at_com)
    a = np.zeros((len(root), NV), F) if accel is None else np.asarray(accel, F)
    return c, DR.evaluate(root, dof, vel_at_com, ms, arm, a, g, dtype=dtype, c=c)["tau"], a


def evaluate(root, dof, vel_at_com, ms, arm, contacts, accel=None, weights=None, f_ref=None, g=None, pre=None):
    """The float64 reference: dict of tau_full, jc, force [N, m], tau_joint [N, 33], contact_accel [N, m]."""
    c, r, a = pre if pre is not None else front(root, dof, vel_at_com, ms, arm, accel, np.float64, g)
    J = CR.jc_of(c, contacts, vel_at_com)
    N, m = J.shape[0], J.shape[1]
    w = weights_of(weights, m // 6)
    fr = np.zeros((N, m)) if f_ref is None else np.asarray(f_ref, F).astype(np.float64)
    Jb = J[:, :, 0:6]
    rhs = r[:, 0:6] - np.einsum("nrk,nr->nk", Jb, fr)
    f = np.empty((N, m))
    for e in range(N):
        z = np.linalg.lstsq(Jb[e].T / np.sqrt(w), rhs[e], rcond=None)[0]
        f[e] = fr[e] + z / np.sqrt(w)
    tj = r[:, 6:] - np.einsum("nrj,nr->nj", J[:, :, 6:], f)
    return {"tau_full": r, "jc": J, "force": f, "tau_joint": tj, "contact_accel": contact_accel_of(c, dof, contacts, vel_at_com, a.astype(np.float64)),
            "weights": w, "f_ref": fr}


def restate(root, dof, vel_at_com, ms, arm, contacts, accel=None, weights=None, f_ref=None, g=None, dtype=np.float32, pre=None):
    """The same dict by the header's arithmetic in its order, in one number format."""
    c, r, a = pre if pre is not None else front(root, dof, vel_at_com, ms, arm, accel, dtype, g)
    J = CR.jc_of(c, contacts, vel_at_com)
    N, m = J.shape[0], J.shape[1]
    w = weights_of(weights, m // 6, dtype)
    fr = np.zeros((N, m), dtype) if f_ref is None else np.asarray(f_ref, F).astype(dtype)
    G = np.zeros((N, 6, 6), dtype)
    for i in range(6):
        for j in range(i + 1):
            v = np.zeros(N, dtype)
            for k in range(m):
                v = v + (J[:, k, i] / w[k]) * J[:, k, j]
            G[:, i, j] = G[:, j, i] = v
    s = np.zeros((N, 6), dtype)
    for k in range(m):
        s = s + J[:, k, 0:6] * fr[:, k, None]
    L, D = CR.ldl(G)
    y = CR.small_solve(L, D, (r[:, 0:6] - s)[:, None, :])[:, 0]
    t = np.zeros((N, m), dtype)
    for k in range(6):
        t = t + J[:, :, k] * y[:, k, None]
    f = fr + t / w
    s = np.zeros((N, 33), dtype)
    for k in range(m):
        s = s + J[:, k, 6:] * f[:, k, None]
    return {"tau_full": r, "jc": J, "G": G, "force": f, "tau_joint": r[:, 6:] - s, "contact_accel": contact_accel_of(c, dof, contacts, vel_at_com, a.astype(dtype))}


def split(out):
    ch = {}
    if out.get("force") is not None:
        x = out["force"].reshape(out["force"].shape[0], -1, 6)
        ch["force_f"], ch["force_n"] = x[..., 0:3], x[..., 3:6]
    if out.get("tau_joint") is not None:
        ch["tau_joint"] = out["tau_joint"]
    if out.get("contact_accel") is not None:
        x = out["contact_accel"].reshape(out["contact_accel"].shape[0], -1, 6)
        ch["ca_lin"], ch["ca_ang"] = x[..., 0:3], x[..., 3:6]
    return ch


def _wkey(weights):
    return None if weights is None else tuple(float(x) for x in np.asarray(weights, F).reshape(-1))


@functools.lru_cache(maxsize=None)
def _measured_state(vel_at_com):
    root, dof, ms, arm, acc = DR.seeded(STATES, 27000 + 10 * vel_at_com)
    return root, dof, ms, arm, front(root, dof, vel_at_com, ms, arm, acc, np.float64), front(root, dof, vel_at_com, ms, arm, acc, np.float32)


@functools.lru_cache(maxsize=None)
def _measured(vel_at_com, K, wkey, with_ref):
    root, dof, ms, arm, pre64, pre32 = _measured_state(vel_at_com)
    fr = fref_of(STATES, 6 * K, 27007) if with_ref else None
    want = evaluate(root, dof, vel_at_com, ms, arm, SETS[K], None, wkey, fr, pre=pre64)
    a, b = split(want), split(restate(root, dof, vel_at_com, ms, arm, SETS[K], None, wkey, fr, pre=pre32))
    d = {ch: float(np.abs(a[ch] - b[ch].astype(np.float64)).max()) for ch in CHANNELS}
    d["force_scale"], d["tau_joint_scale"] = float(np.abs(want["force"]).max()), float(np.abs(want["tau_joint"]).max())
    Jb = want["jc"][:, :, 0:6]
    d["cond"] = float(np.linalg.cond(np.einsum("nri,r,nrj->nij", Jb, 1.0 / want["weights"], Jb)).max())
    return d


def measured(vel_at_com, K, weights=None, with_ref=False):
    """d per channel, the largest force and tau_joint words it was measured with, and the largest cond(G)."""
    return _measured(int(bool(vel_at_com)), K, _wkey(weights), bool(with_ref))


def allowance(want, vel_at_com, K, kind, weights=None, with_ref=False):
    """FACTOR * d per word of force [N, m], tau_joint [N, 33] or contact_accel [N, m] of a float64 reference dict; force's and tau_joint's
    scaled with the solution."""
    d = measured(vel_at_com, K, weights, with_ref)
    if kind == "contact_accel":
        return FACTOR * np.broadcast_to(np.array(([d["ca_lin"]] * 3 + [d["ca_ang"]] * 3) * K), want[kind].shape)
    s = np.maximum(1.0, np.abs(want[kind]).max(-1, keepdims=True) / d[kind + "_scale"])
    own = np.array(([d["force_f"]] * 3 + [d["force_n"]] * 3) * K) if kind == "force" else np.full(33, d["tau_joint"])
    return FACTOR * own * s


def excess(got, want, vel_at_com, K, weights=None, with_ref=False, report=None):
    """Every channel of the outputs in dict `got` (any subset of tau_joint, force, contact_accel) against the float64 reference dict `want`,
    as the largest deviation divided by its allowance: a dict channel -> ratio; all must be <= 1."""
    out = {}
    for kind in ("force", "tau_joint", "contact_accel"):
        if got.get(kind) is None:
            continue
        have = np.asarray(got[kind], F).astype(np.float64).reshape(want[kind].shape)
        ratio = np.abs(have - want[kind]) / allowance(want, vel_at_com, K, kind, weights, with_ref)
        for ch, x in split({kind: ratio}).items():
            out[ch] = float(x.max())
    if report is not None:
        print(report, {k: round(v, 3) for k, v in out.items()}, "d:", {k: "%.2e" % v for k, v in measured(vel_at_com, K, weights, with_ref).items()})
    return out


def within(ex: dict) -> bool:
    return len(ex) > 0 and all(np.isfinite(v) and v <= 1.0 for v in ex.values())
