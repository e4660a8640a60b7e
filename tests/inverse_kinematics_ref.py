"""The inverse kinematics restated in numpy from the rules of include/dyros_inverse_kinematics.h, on top of
tests/body_states_ref.py's chain and tests/contact_dynamics_ref.py's Jacobian at a body's point (jc_of); shared by
tests/test_inverse_kinematics.py (the g++ build of csrc/dw_inverse_kinematics.h) and tests/test_inverse_kinematics_gpu.py (the HIP kernel).
Test helper.

step() is one update in float64 and does NOT take the normal equations the kernel uses: dnu is what np.linalg.lstsq gives for the stacked
system  [W^1/2 J; lambda I] dnu = [W^1/2 e; 0].  solve() is the loop around it with the header's stopping rule.  restate() is the header's
arithmetic in its order (A = J J' + lambda^2 W^-1 summed over the columns ascending, contact_dynamics_ref's L D L' and sweeps, dnu = J' y
summed over the rows ascending, the step limit, the update) in one number format, with faults that can be injected.

The tolerance is measured here, against the reference and never against a kernel (tests/body_states_ref.py's method): per channel, d = the
largest deviation of the float32 restatement from the float64 reference over STATES seeded cases of the same construction as the tests'
(case()); what is tested must be within FACTOR * d.  Channels: q (the masked joints), res_pos / res_ang (the residual rows as returned),
rq_pos / rq_ang (the residual rows recomputed in float64 from the returned q and base), base_pos, base_R (the base's rotation matrix).
"""
import functools

import numpy as np

import body_states_ref as R
import contact_dynamics_ref as CR
import jacobians_ref as JR

NV, ND = 39, 33
FACTOR, STATES = R.FACTOR, R.STATES
F = np.float32
SETS = CR.SETS
LOWER, UPPER = np.asarray(R.MODEL.dof_lower, F), np.asarray(R.MODEL.dof_upper, F)
ORI_10 = (1.0, 1.0, 1.0, 10.0, 10.0, 10.0)
KINDS = {"pose": (1,) * 6, "position": (1, 1, 1, 0, 0, 0), "orientation": (0, 0, 0, 1, 1, 1)}
CHANNELS = ("q", "res_pos", "res_ang", "rq_pos", "rq_ang", "base_pos", "base_R")
OUTS = ("q", "root", "residual", "err", "iters", "converged")
FAULTS = ("drop_row", "drop_column", "skip_clamp")


def path_dofs(contacts):
    """The Gym DoFs on the paths from the base to the targets' bodies, ascending: the default DoF mask."""
    return sorted({b - 1 for m in CR.carriers(contacts) for b in JR.ANC[m]})


def problem(K=2, rows=None, weights=None, dofs=None, base=False, iterations=16, damping=0.05, max_step=0.5, tol_pos=1e-5, tol_ang=1e-5, limits=True,
            rel_root=False, contacts=None):
    """A solver's settings as a dict: rows per target "pose" | "position" | "orientation" (None: poses), weights None, six numbers or [m]."""
    cs = SETS[K] if contacts is None else tuple(contacts)
    k = len(cs)
    rmask = np.array([b for kind in (rows or ("pose",) * k) for b in KINDS[kind]], bool)
    w = np.ones(6 * k, F) if weights is None else (np.tile(np.asarray(weights, F), k) if np.size(weights) == 6 else np.asarray(weights, F).reshape(6 * k))
    ids = path_dofs(cs) if dofs is None else sorted(int(j) for j in dofs)
    dmask = np.zeros(ND, bool)
    dmask[ids] = True
    return {"contacts": cs, "K": k, "m": 6 * k, "rows": rmask, "w": w, "dofs": dmask, "base": bool(base), "iterations": int(iterations),
            "damping": F(damping), "max_step": F(max_step), "tol_pos": F(tol_pos), "tol_ang": F(tol_ang), "limits": bool(limits), "rel_root": bool(rel_root)}


def cols_of(P):
    return np.concatenate([np.full(6, P["base"]), P["dofs"]])


def forward(root, q, P, dtype=np.float64):
    """(chain, the points' offsets from the base [N, K, 3], the bodies' quaternions [N, K, 4]) at (base, q)."""
    dof = np.zeros((len(root), ND, 2), dtype)
    dof[:, :, 0] = q
    c = R.chain(root, dof, dtype, 0)
    m = CR.carriers(P["contacts"])
    return c, c["off"][:, m] + CR.arms(c, P["contacts"]), c["q"][:, m]


def targets_of(root, q, P):
    """targets [N, K, 7] float32 of the bodies' poses at (base, q), by the float64 chain: what the solver reaches with no update."""
    c, pt, qb = forward(root, q, P)
    pos = pt if P["rel_root"] else c["root"][:, None, 0:3] + pt
    return np.concatenate([pos, qb], -1).astype(F)


def errors(c, pt, qb, tgt, P):
    """(e [N, m] with +0 on inactive rows, dead [N]) in the chain's number format."""
    dt = pt.dtype
    t = np.asarray(tgt).astype(dt)
    lin = (t[..., 0:3] if P["rel_root"] else t[..., 0:3] - c["root"][:, None, 0:3]) - pt
    n = np.sqrt(t[..., 3] * t[..., 3] + t[..., 4] * t[..., 4] + t[..., 5] * t[..., 5] + t[..., 6] * t[..., 6])
    qc = qb * np.array([-1, -1, -1, 1], dt)
    with np.errstate(all="ignore"):
        qe = R.qmul(t[..., 3:7] / n[..., None], qc)
    ang = dt.type(2) * np.where(qe[..., 3:4] < 0, -qe[..., 0:3], qe[..., 0:3])
    e = np.concatenate([lin, ang], -1).reshape(len(pt), -1)
    e = np.where(P["rows"], e, dt.type(0))
    with np.errstate(invalid="ignore"):
        dead = ~((n >= F(0.99)) & (n <= F(1.01))).all(-1) | ~np.isfinite(e).all(-1)
    return e, dead


def tol_of(P):
    return np.tile(np.array([P["tol_pos"]] * 3 + [P["tol_ang"]] * 3), P["K"])


def jac_of(c, P):
    """J [N, m, 39] with zeros in the inactive rows and the held columns."""
    J = CR.jc_of(c, P["contacts"], 0)
    return J * P["rows"][None, :, None] * cols_of(P)[None, None, :]


def dnu_lstsq(J, e, P):
    """float64: the stacked system's least-squares solution, env by env."""
    sw, lam = np.sqrt(P["w"].astype(np.float64)), float(P["damping"])
    out = np.zeros((len(J), NV))
    for n in range(len(J)):
        if np.isfinite(J[n]).all() and np.isfinite(e[n]).all():
            out[n] = np.linalg.lstsq(np.concatenate([sw[:, None] * J[n], lam * np.eye(NV)]), np.concatenate([sw * e[n], np.zeros(NV)]), rcond=None)[0]
    return out


def a_of(J, P):
    """A = J J' + lambda^2 W^-1 in J's number format, the columns summed ascending; an inactive row's diagonal is 1."""
    dt = J.dtype
    m = J.shape[1]
    A = np.zeros((len(J), m, m), dt)
    for c in range(NV):
        A = A + J[:, :, None, c] * J[:, None, :, c]
    lam, w = dt.type(P["damping"]), P["w"].astype(dt)
    i = np.arange(m)
    A[:, i, i] = np.where(P["rows"], A[:, i, i] + (lam * lam) / w, dt.type(1))
    return A


def dnu_normal(J, e, P):
    """The header's order in J's number format."""
    with np.errstate(all="ignore"):
        L, D = CR.ldl(a_of(J, P))
        y = CR.small_solve(L, D, e[:, None, :])[:, 0]
        out = np.zeros((len(J), NV), J.dtype)
        for r in range(J.shape[1]):
            out = out + J[:, r, :] * y[:, r, None]
    return out


def base_update(root, dv):
    dt = root.dtype
    q = root[:, 3:7] / np.sqrt((root[:, 3:7] * root[:, 3:7]).sum(-1, dtype=dt))[:, None]
    o = R.qmul(np.concatenate([dt.type(0.5) * dv[:, 3:6], np.ones((len(root), 1), dt)], -1), q)
    out = root.copy()
    out[:, 0:3] = root[:, 0:3] + dv[:, 0:3]
    out[:, 3:7] = o / np.sqrt((o * o).sum(-1, dtype=dt))[:, None]
    return out


def solve(root, q0, tgt, P, dtype=np.float64, normal=False, fault=None):
    """The loop: dict of q [N, 33], root [N, 7], residual [N, m], err [N, 2], iters [N], converged [N], dead [N] and the iterate's full
    root rows "root13".  normal: the kernel's normal equations in its order (restate) instead of lstsq; fault: one of FAULTS (normal only)."""
    dt = np.dtype(dtype)
    root, q = np.asarray(root, F).astype(dt), np.asarray(q0, F).astype(dt)
    N, tol = len(root), tol_of(P)
    iters, dead = np.zeros(N, np.int32), np.zeros(N, bool)
    lo, hi, lim = LOWER.astype(dt), UPPER.astype(dt), dt.type(P["max_step"])

    def look():
        c, pt, qb = forward(root, q, P, dt)
        e, bad = errors(c, pt, qb, tgt, P)
        with np.errstate(invalid="ignore"):
            done = (~P["rows"] | (np.abs(e) <= tol)).all(-1)
        return c, e, bad, done

    for _ in range(P["iterations"]):
        c, e, bad, done = look()
        dead |= bad
        mv = ~dead & ~done
        if not mv.any():
            break
        J = jac_of(c, P)
        if fault == "drop_row":
            r = int(np.flatnonzero(P["rows"])[-1])
            J[:, r], e = 0, np.where(np.arange(P["m"]) == r, dt.type(0), e)
        if fault == "drop_column":
            J[:, :, int(np.flatnonzero(cols_of(P))[-1])] = 0
        dv = (dnu_normal(J, e, P) if normal else dnu_lstsq(J, e, P)).astype(dt)
        with np.errstate(all="ignore"):
            big = np.abs(dv[:, 6:]).max(-1)
            dv = dv * np.where(big > lim, lim / big, dt.type(1))[:, None]
            qn = q + dv[:, 6:]
            if P["limits"] and fault != "skip_clamp":
                qn = np.where(qn < lo, lo, np.where(qn > hi, hi, qn))
        q = np.where(mv[:, None] & P["dofs"], qn, q)
        if P["base"]:
            root = np.where(mv[:, None], base_update(root, dv), root)
        iters += mv
    _c, e, bad, done = look()
    dead |= bad
    nan = np.where(dead, np.nan, 1.0).astype(dt)[:, None]
    pos = np.where(P["rows"] & (np.arange(P["m"]) % 6 < 3), np.abs(e), 0).max(-1)
    ang =np.where(P["rows"] & (np.arange(P["m"]) % 6 >= 3), np.abs(e), 0).max(-1)
    return {"q": q * nan, "root": root[:, 0:7] * nan, "root13": root, "residual": e * nan, "err": np.stack([pos, ang], -1) * nan,
            "iters": np.where(dead, 0, iters).astype(np.int32), "converged": (done & ~dead).astype(np.uint8), "dead": dead}


def step(root, q0, tgt, P):
    """One update in float64 by lstsq: the arithmetic's pin."""
    return solve(root, q0, tgt, dict(P, iterations=1))


def restate(root, q0, tgt, P, dtype=np.float32, fault=None):
    """The header's order in one number format."""
    return solve(root, q0, tgt, P, dtype, normal=True, fault=fault)


def residual64(out, root, tgt, P):
    """The error rows in float64 at an output's q and base pose (root: the input rows, whose velocities are not read)."""
    r = np.asarray(root, F).astype(np.float64)
    if out.get("root") is not None:
        r = np.concatenate([np.asarray(out["root"]).astype(np.float64), r[:, 7:]], -1)
    c, pt, qb = forward(r, np.asarray(out["q"]).astype(np.float64), P)
    return errors(c, pt, qb, tgt, P)[0]


def case(n, seed, P, delta=0.3):
    """(root [n, 13], q0 [n, 33], targets [n, K, 7], q* [n, 33]) float32: seeded states, and the targets the float64 chain reaches at q* =
    clip(q0 + d), d uniform within +-delta on the masked joints: reachable inside the limits."""
    root, dof, _ = R.states(n, seed)
    q0 = np.ascontiguousarray(dof[:, :, 0])
    d = np.random.default_rng(seed + 1).uniform(-delta, delta, (n, ND)) * P["dofs"]
    qs = np.clip(q0 + d.astype(F), LOWER, UPPER).astype(F)
    return root, q0, targets_of(root, qs, P), qs


# the convergence cases of both test files: CONV_N cases (3 G + 2 for the kernel's group of 4) of seed CONV_SEED, at most 8 updates with
# lambda = 0.01.  With the default 0.05 the seeded states, whose joints are drawn uniformly up to +-1.5 rad, pass near enough to a straight
# knee or an aligned hip that the damping's linear rate lambda^2 / (sigma^2 + lambda^2) leaves 29 to 45 % of 256 fixed-base cases short of
# 1e-5 after 16 updates; at 0.01 seed 103 is the first whose 14 cases all converge in float64 within 8, for one, two and four targets
CONV_N, CONV_SEED, CONV = 14, 103, {"iterations": 8, "damping": 0.01}
MIXED = {1: ("position",), 2: ("pose", "position"), 4: ("pose", "position", "orientation", "pose")}          # row masks of the one-step tests


@functools.lru_cache(maxsize=None)
def conv_case(K, base):
    """(P, root, q0, targets, the float64 reference's outputs) of the convergence cases, computed once."""
    P = problem(K, base=base, **CONV)
    root, q0, tgt, _ = case(CONV_N, CONV_SEED, P)
    return P, root, q0, tgt, solve(root, q0, tgt, P)


def split(out, root=None, tgt=None, P=None):
    """An output dict as channels; with root, tgt and P also the residual recomputed in float64."""
    ch = {}
    f = lambda x: np.asarray(x).astype(np.float64)          # noqa: E731
    if out.get("q") is not None:
        ch["q"] = f(out["q"])[:, P["dofs"]]
    if out.get("residual") is not None:
        x = f(out["residual"]).reshape(len(out["residual"]), -1, 6)
        ch["res_pos"], ch["res_ang"] = x[..., 0:3], x[..., 3:6]
    if out.get("q") is not None and root is not None:
        x = residual64(out, root, tgt, P).reshape(len(root), -1, 6)
        ch["rq_pos"], ch["rq_ang"] = x[..., 0:3], x[..., 3:6]
    if out.get("root") is not None:
        ch["base_pos"], ch["base_R"] = f(out["root"])[:, 0:3], R.qmat(f(out["root"])[:, 3:7])
    return ch


def _key(P):
    return (P["contacts"], tuple(P["rows"]), tuple(float(x) for x in P["w"]), tuple(P["dofs"]), P["base"], P["iterations"], float(P["damping"]), float(P["max_step"]),
            float(P["tol_pos"]), float(P["tol_ang"]), P["limits"], P["rel_root"])


_cache = {}


def measured(P):
    """d per channel for the settings P: the float32 restatement against the float64 reference at STATES seeded cases; "unconverged": how many
    of them the reference left unconverged."""
    k = _key(P)
    if k not in _cache:
        root, q0, tgt, _ = case(STATES, 29000, P)
        want = solve(root, q0, tgt, P)
        a, b = split(want, root, tgt, P), split(restate(root, q0, tgt, P), root, tgt, P)
        d = {ch: float(np.abs(a[ch] - b[ch]).max()) for ch in CHANNELS}
        d["unconverged"] = int((want["converged"] == 0).sum())
        _cache[k] = d
    return _cache[k]


def excess(got, want, root, tgt, P, report=None):
    """Every channel of the outputs in dict `got` (q, root, residual, each or None) against the float64 reference dict `want`, as the largest
    deviation divided by FACTOR * d: a dict channel -> ratio; all must be <= 1 (a channel whose d is 0 -- bits -- allows no deviation)."""
    d = measured(P)
    a, b = split(want, root, tgt, P), split(got, root if got.get("q") is not None else None, tgt, P)
    out = {}
    for ch in b:
        dev = float(np.abs(a[ch] - b[ch]).max()) if np.isfinite(b[ch]).all() else np.inf
        out[ch] = dev / (FACTOR * d[ch]) if d[ch] > 0 else (0.0 if dev == 0 else np.inf)
    if report is not None:
        print(report, {k: round(v, 3) for k, v in out.items()}, "d:", {k: "%.2e" % v for k, v in d.items() if k in CHANNELS})
    return out


def within(ex: dict) -> bool:
    return len(ex) > 0 and all(np.isfinite(v) and v <= 1.0 for v in ex.values())


@functools.lru_cache(maxsize=None)
def cond_of(K, damping, base=False, weights=None):
    """The largest cond(A) over the STATES seeded states at q0."""
    P = problem(K, weights=weights, base=base, damping=damping)
    root, q0, _tgt, _ = case(STATES, 29000, P)
    c = forward(root, q0, P)[0]
    return float(np.linalg.cond(a_of(jac_of(c, P), P)).max())
