"""The stance inverse dynamics restated in numpy from the rules of include/dyros_stance_inverse_dynamics.h, on top of
tests/contact_inverse_dynamics_ref.py; shared by tests/test_stance_inverse_dynamics.py (the g++ build of csrc/dw_stance_inverse.h) and
tests/test_stance_inverse_dynamics_gpu.py (the HIP kernel).  Test helper.

The reference is float64 and is held against what it is not itself: an env's force and tau_joint are
contact_inverse_dynamics_ref.evaluate's (np.linalg.lstsq, not the normal equations) on the SUBSET of the contacts that the env's stance
names, with that subset's weights and f_ref; an env in flight gets force 0, tau_joint = r[6:] and base_residual = r[0:6].  The margins are
restated from tests/body_states_ref.py's rotations.

The tolerance is measured here, against the reference and never against a kernel (section 21's method): per channel, d = the largest
deviation of the float32 restatement (contact_inverse_dynamics_ref.restate on the subset, then the header's order for base_residual and the
margins) from the float64 reference over STATES seeded states, for each velocity mode, K = 2 (env e takes pattern e mod 4: every pattern)
and K = 4 (a seeded mix of the 16 patterns), unit weights and moments weighted 10 x, with or without f_ref; what is tested must be within
FACTOR * d.  force, tau_joint, the margins (linear in f) and base_residual (rounding of sums of |r|'s size; r[0:6] itself in flight) grow
with the solution: an env whose largest word is s times the largest that d was measured with gets s d.  Channels: force_f, force_n,
tau_joint, ca_lin, ca_ang, base_lin, base_ang, margin_n, margin_mu, margin_cx, margin_cy.
"""
import functools

import numpy as np

import body_states_ref as R
import contact_dynamics_ref as CR
import contact_inverse_dynamics_ref as IR

NV = 39
FACTOR, STATES = R.FACTOR, R.STATES
F = np.float32
SETS = CR.SETS
CHANNELS = IR.CHANNELS + ("base_lin", "base_ang", "margin_n", "margin_mu", "margin_cx", "margin_cy")
OUTS = IR.OUTS + ("base_residual", "margins", "feasible")
MOMENTS_10 = IR.MOMENTS_10
MODEL_SOLE = (0.03, 0.0, -0.1585, 0.15, 0.085)          # the bounding rectangle of a foot's four foot_pts (tocabi_model.json)
FOOT_MOVING = sorted({f["moving"] for f in R.MODEL.d["foot_pts"]})


def soles_of(contacts):
    """[K, 5] float32: the model's sole for a contact on a foot, a point at its pos otherwise ("soles": "model")."""
    return np.array([MODEL_SOLE if b in FOOT_MOVING else tuple(pos) + (0.0, 0.0) for b, (_, pos) in zip(CR.carriers(contacts), contacts)], F)


def stance_cycle(n, K, s=0):
    """[n, K] uint8: env e takes pattern (e + s) mod 2^K, bit i for contact i."""
    p = (np.arange(n) + s) % (1 << K)
    return ((p[:, None] >> np.arange(K)) & 1).astype(np.uint8)


def stance_mix(n, K, seed):
    """[n, K] uint8: seeded patterns, every one of the 2^K among them."""
    p = np.random.default_rng(seed).integers(0, 1 << K, n)
    p[:1 << K] = np.arange(1 << K)
    return ((p[:, None] >> np.arange(K)) & 1).astype(np.uint8)


def margins_of(c, contacts, force, stance, soles, mu, dtype):
    """[N, K, 4] in one number format, in the header's order, from the chain's rotations; +0.0 for an inactive contact."""
    N, K = stance.shape
    Rb = c["R"][:, CR.carriers(contacts)].astype(dtype)          # [N, K, 3, 3]
    w = force.astype(dtype).reshape(N, K, 6)
    so, pos, mu = np.asarray(soles, F).astype(dtype), np.array([p for _, p in contacts], F).astype(dtype), dtype(F(mu))
    fb = [Rb[:, :, 0, a] * w[:, :, 0] + Rb[:, :, 1, a] * w[:, :, 1] + Rb[:, :, 2, a] * w[:, :, 2] for a in range(3)]
    mb = [Rb[:, :, 0, a] * w[:, :, 3] + Rb[:, :, 1, a] * w[:, :, 4] + Rb[:, :, 2, a] * w[:, :, 5] for a in range(3)]
    d = [so[None, :, a] - pos[None, :, a] for a in range(3)]
    msx, msy = mb[0] - (d[1] * fb[2] - d[2] * fb[1]), mb[1] - (d[2] * fb[0] - d[0] * fb[2])
    out = np.stack([fb[2], mu * fb[2] - np.sqrt(fb[0] * fb[0] + fb[1] * fb[1]), so[None, :, 3] * fb[2] - np.abs(msy), so[None, :, 4] * fb[2] - np.abs(msx)], -1)
    return np.where(stance[:, :, None] != 0, out, dtype(0.0))


def _solve(fn, dtype, root, dof, vel_at_com, ms, arm, contacts, stance, accel, weights, f_ref, soles, mu, g, pre):
    """fn: contact_inverse_dynamics_ref's evaluate or restate, called once per stance pattern on the pattern's envs and contact subset."""
    K = len(contacts)
    stance = (np.ones((len(root), K), np.uint8) if stance is None else np.asarray(stance).reshape(len(root), K) != 0).astype(np.uint8)
    c, r, a = pre if pre is not None else IR.front(root, dof, vel_at_com, ms, arm, accel, dtype, g)
    N, m = len(r), 6 * K
    W = IR.weights_of(weights, K, dtype).reshape(K, 6)
    fr = np.zeros((N, m), F) if f_ref is None else np.asarray(f_ref, F).reshape(N, m)
    force, tj, base = np.zeros((N, m), dtype), np.array(r[:, 6:], copy=True), np.array(r[:, 0:6], copy=True)
    J = CR.jc_of(c, contacts, vel_at_com)
    code = (stance.astype(np.int64) << np.arange(K)).sum(1)
    for p in np.unique(code):
        if p == 0:
            continue          # (flight: nothing is solved)
        idx, S = np.nonzero(code == p)[0], [i for i in range(K) if (p >> i) & 1]
        rows = np.concatenate([np.arange(6 * i, 6 * i + 6) for i in S])
        sub = fn(None, np.asarray(dof)[idx], vel_at_com, None, None, tuple(contacts[i] for i in S), None, W[S], fr[idx][:, rows],
                 pre=({k: x[idx] for k, x in c.items()}, r[idx], a[idx]))
        force[np.ix_(idx, rows)] = sub["force"]
        tj[idx] = sub["tau_joint"]
        # base_residual in the header's order: r[k] minus the sum over the active rows ascending
        s = np.zeros((len(idx), 6), dtype)
        for k in rows:
            s = s + J[idx, k, 0:6] * force[idx, k, None]
        base[idx] = r[idx, 0:6] - s
    so = soles_of(contacts) if soles is None else np.asarray(soles, F).reshape(K, 5)
    mg = margins_of(c, contacts, force, stance, so, mu, dtype)
    feasible = ((code != 0) & np.where(stance[:, :, None] != 0, mg >= 0, True).all((1, 2))).astype(np.uint8)
    return {"tau_full": r, "jc": J, "force": force, "tau_joint": tj, "contact_accel": IR.contact_accel_of(c, dof, contacts, vel_at_com, a.astype(dtype)),
            "base_residual": base, "margins": mg, "feasible": feasible, "stance": stance}


def evaluate(root, dof, vel_at_com, ms, arm, contacts, stance=None, accel=None, weights=None, f_ref=None, soles=None, mu=1.0, g=None, pre=None):
    """The float64 reference: dict of tau_full, jc, force [N, m], tau_joint [N, 33], contact_accel [N, m], base_residual [N, 6], margins [N,
    K, 4], feasible [N].  stance [N, K] (None: ones); soles [K, 5] (None: soles_of)."""
    return _solve(IR.evaluate, np.float64, root, dof, vel_at_com, ms, arm, contacts, stance, accel, weights, f_ref, soles, mu, g, pre)


def restate(root, dof, vel_at_com, ms, arm, contacts, stance=None, accel=None, weights=None, f_ref=None, soles=None, mu=1.0, g=None, dtype=np.float32,
            pre=None):
    """The same dict by the header's arithmetic in its order, in one number format."""
    return _solve(lambda *a, **k: IR.restate(*a, dtype=dtype, **k), dtype, root, dof, vel_at_com, ms, arm, contacts, stance, accel, weights, f_ref, soles, mu,
                  g, pre)


def split(out):
    ch = IR.split(out)
    if out.get("base_residual") is not None:
        ch["base_lin"], ch["base_ang"] = out["base_residual"][:, 0:3], out["base_residual"][:, 3:6]
    if out.get("margins") is not None:
        for i, k in enumerate(("margin_n", "margin_mu", "margin_cx", "margin_cy")):
            ch[k] = out["margins"][..., i]
    return ch


def measured_stance(K):
    return stance_cycle(STATES, K) if K == 2 else stance_mix(STATES, K, 28003)


@functools.lru_cache(maxsize=None)
def _measured(vel_at_com, K, wkey, with_ref):
    root, dof, ms, arm, pre64, pre32 = IR._measured_state(vel_at_com)
    fr = IR.fref_of(STATES, 6 * K, 28007) if with_ref else None
    st = measured_stance(K)
    want = evaluate(root, dof, vel_at_com, ms, arm, SETS[K], st, None, wkey, fr, pre=pre64)
    a, b = split(want), split(restate(root, dof, vel_at_com, ms, arm, SETS[K], st, None, wkey, fr, pre=pre32))
    d = {ch: float(np.abs(a[ch] - b[ch].astype(np.float64)).max()) for ch in CHANNELS}
    d["force_scale"], d["tau_joint_scale"] = float(np.abs(want["force"]).max()), float(np.abs(want["tau_joint"]).max())
    d["base_scale"] = float(np.abs(want["tau_full"][:, 0:6]).max())
    return d


def measured(vel_at_com, K, weights=None, with_ref=False):
    """d per channel and the largest force, tau_joint and r[0:6] words it was measured with."""
    return _measured(int(bool(vel_at_com)), K, IR._wkey(weights), bool(with_ref))


def allowance(want, vel_at_com, K, kind, weights=None, with_ref=False):
    """FACTOR * d per word of an output of a float64 reference dict; all but contact_accel's scaled with the solution."""
    d = measured(vel_at_com, K, weights, with_ref)
    if kind == "contact_accel":
        return FACTOR * np.broadcast_to(np.array(([d["ca_lin"]] * 3 + [d["ca_ang"]] * 3) * K), want[kind].shape)
    sf = np.maximum(1.0, np.abs(want["force"]).max(-1, keepdims=True) / d["force_scale"])
    if kind == "force":
        return FACTOR * np.array(([d["force_f"]] * 3 + [d["force_n"]] * 3) * K) * sf
    if kind == "margins":
        return FACTOR * np.array([d["margin_n"], d["margin_mu"], d["margin_cx"], d["margin_cy"]])[None, None, :] * sf[:, :, None]
    if kind == "base_residual":
        return FACTOR * np.array([d["base_lin"]] * 3 + [d["base_ang"]] * 3) * np.maximum(1.0, np.abs(want["tau_full"][:, 0:6]).max(-1, keepdims=True) / d["base_scale"])
    return FACTOR * np.full(33, d["tau_joint"]) * np.maximum(1.0, np.abs(want["tau_joint"]).max(-1, keepdims=True) / d["tau_joint_scale"])


def excess(got, want, vel_at_com, K, weights=None, with_ref=False, report=None):
    """Every channel of the outputs in dict `got` (any subset of force, tau_joint, contact_accel, base_residual, margins) against the float64
    reference dict `want`, as the largest deviation divided by its allowance: a dict channel -> ratio; all must be <= 1."""
    out = {}
    for kind in ("force", "tau_joint", "contact_accel", "base_residual", "margins"):
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
