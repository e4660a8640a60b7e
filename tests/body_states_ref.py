"""The rigid-body state tensor restated in numpy (include/dyros_bodies.h), shared by tests/test_body_states.py (the g++
build of csrc/dw_bodies.h) and tests/test_body_states_gpu.py (the HIP kernel).  Test helper, in the style of tests/gait_profile_ref.py.

chain(root, dof, dtype) is the recursion of the header in one number format: float64 is the reference, float32 the measure of what the format
costs.  Both are evaluated at the same float32 inputs; the model constants are the JSON's in float64 and their float32 roundings (what the
device table holds) in float32, so d includes what rounding the constants costs.

The tolerance is measured here, against the reference and never against a kernel: per channel, d = the largest deviation of the float32 recursion
from the float64 one over STATES seeded states, and what is tested must be within FACTOR * d.  The margin of four covers a different summation
order and OCML's sinf / cosf against libm's, a few ulp each; an indexing, sign or frame mistake is three orders of magnitude larger than d.
An absolute position is held to FACTOR * d_offset + one float32 ulp of |x| per coordinate (the base is added last, with one rounding).
Quaternions are compared through R(q), so the sign is free; |norm(q) - 1| is a channel of its own.
"""
import functools

import numpy as np

from isaacgymdyros_amd.model import load_model

MODEL = load_model()
NB, NM, NI = 38, 34, 36
FACTOR, STATES = 4.0, 4096
F = np.float32


# ---------------------------------------------------------------------------------------------- quaternions, xyzw
def qmul(a, b):
    ax, ay, az, aw = (a[..., i] for i in range(4))
    bx, by, bz, bw = (b[..., i] for i in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def qmat(q):
    x, y, z, w = (q[..., i] for i in range(4))
    one, two = q.dtype.type(1), q.dtype.type(2)
    return np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y), two * (x * y + w * z), one - two * (x * x + z * z),
                     two * (y * z - w * x), two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def quat_of(R):
    """The unit quaternion xyzw, w > 0 (a half turn: the first non-zero of x, y, z positive), of a rotation matrix, in float64: the eigenvector of the largest eigenvalue of the 4x4 matrix K(R)."""
    R = np.asarray(R, np.float64)
    Kq = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                   [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                   [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                   [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(Kq)
    q = v[:, np.argmax(w)]
    lead = [c for c in (q[3], q[0], q[1], q[2]) if abs(c) > 1e-6][0]          # (a half turn has w = 0: then the first of x, y, z)
    return q if lead > 0 else -q


# the model in float64 (rot0 as a quaternion); chain() rounds it to the number format it runs in, as the device table rounds it to float32
MV_PARENT = list(MODEL.mv_parent)
MV_POS = np.asarray(MODEL.mv_pos, np.float64)
MV_AXIS = np.asarray(MODEL.mv_axis, np.float64)
MV_Q0 = np.stack([quat_of(r) for r in MODEL.mv_rot0])
CARRIER = list(MODEL.body_moving)
INERT_GYM, INERT_MV = list(MODEL.inert_gym), list(MODEL.inert_mv)
INERT_MASS = np.asarray(MODEL.inert_mass, np.float64)
INERT_COM = np.asarray(MODEL.inert_com, np.float64)
RECORD = [INERT_GYM.index(g) if g in INERT_GYM else -1 for g in range(NB)]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def mv3(R, v):
    """R [..., 3, 3] times v ([3] or [..., 3]), summed left to right as the C code does."""
    return np.stack([R[..., i, 0] * v[..., 0] + R[..., i, 1] * v[..., 1] + R[..., i, 2] * v[..., 2] for i in range(3)], -1)


def chain(root, dof, dtype=np.float64, vel_at_com=0, base_first=False):
    """The moving bodies' states in one number format: dict of off [N,34,3] (offset from the base; with base_first the base is added FIRST and
    this is the absolute position, the form the header rules out), q [N,34,4], R [N,34,3,3], vo [N,34,3] (origin velocity), w [N,34,3]."""
    T = np.dtype(dtype).type
    root, dof = np.asarray(root).astype(dtype), np.asarray(dof).astype(dtype).reshape(len(root), 33, 2)          # (callers hand float32 states)
    N = len(root)
    pos, axis, q0 = MV_POS.astype(dtype), MV_AXIS.astype(dtype), MV_Q0.astype(dtype)
    off, q, R = np.zeros((N, NM, 3), dtype), np.zeros((N, NM, 4), dtype), np.zeros((N, NM, 3, 3), dtype)
    vo, w = np.zeros((N, NM, 3), dtype), np.zeros((N, NM, 3), dtype)
    n = np.sqrt((root[:, 3:7] * root[:, 3:7]).sum(-1, dtype=dtype))
    q[:, 0] = root[:, 3:7] / n[:, None]
    R[:, 0] = qmat(q[:, 0])
    vo[:, 0], w[:, 0] = root[:, 7:10], root[:, 10:13]
    if base_first:
        off[:, 0] = root[:, 0:3]
    if vel_at_com:
        vo[:, 0] = vo[:, 0] - cross(w[:, 0], mv3(R[:, 0], INERT_COM[RECORD[0]].astype(dtype)))
    for b in range(1, NM):
        p = MV_PARENT[b]
        d = mv3(R[:, p], pos[b])
        off[:, b] = off[:, p] + d
        vo[:, b] = vo[:, p] + cross(w[:, p], d)
        h = T(0.5) * dof[:, b - 1, 0]
        qj = np.concatenate([axis[b][None, :] * np.sin(h)[:, None], np.cos(h)[:, None]], -1)
        q[:, b] = qmul(q[:, p], qmul(np.broadcast_to(q0[b], qj.shape), qj))
        R[:, b] = qmat(q[:, b])
        w[:, b] = w[:, p] + mv3(R[:, b], axis[b]) * dof[:, b - 1, 1][:, None]
    return {"off": off, "q": q, "R": R, "vo": vo, "w": w, "root": root}


def rows(c, vel_at_com=0, ids=None):
    """The output rows of chain c as pieces: off [N,K,3] (without the base), q [N,K,4], R [N,K,3,3], vel [N,K,3], w [N,K,3]."""
    ids = list(range(NB)) if ids is None else list(ids)
    m = [CARRIER[g] for g in ids]
    vel = c["vo"][:, m].copy()
    if vel_at_com:
        for r, g in enumerate(ids):
            if RECORD[g] >= 0:
                cg = INERT_COM[RECORD[g]].astype(c["off"].dtype)
                vel[:, r] = vel[:, r] + cross(c["w"][:, m[r]], mv3(c["R"][:, m[r]], cg))
    return {"off": c["off"][:, m], "q": c["q"][:, m], "R": c["R"][:, m], "vel": vel, "w": c["w"][:, m]}


def com(c, mass_scale=None):
    """(offset of the COM from the base [N,3], COM velocity [N,3], total mass [N]) of chain c."""
    dt = c["off"].dtype
    N = len(c["off"])
    ms = np.ones((N, NB), dt) if mass_scale is None else np.asarray(mass_scale, F).astype(dt)
    sp, sv, sw = np.zeros((N, 3), dt), np.zeros((N, 3), dt), np.zeros(N, dt)
    for k in range(NI):
        m = INERT_MV[k]
        wk = INERT_MASS[k].astype(dt) * ms[:, INERT_GYM[k]]
        rc = mv3(c["R"][:, m], INERT_COM[k].astype(dt))
        sp += wk[:, None] * (c["off"][:, m] + rc)
        sv += wk[:, None] * (c["vo"][:, m] + cross(c["w"][:, m], rc))
        sw += wk
    return sp / sw[:, None], sv / sw[:, None], sw


# ---------------------------------------------------------------------------------------------- inputs
def states(n, seed, xy=1.0, mass=False):
    """Seeded inputs: base z in [0.5, 1.2], x and y uniform in +-xy, random unit quaternions, v ~ N(0,1), w ~ N(0,2), joint angles uniform
    in [max(lower, -1.5), min(upper, 1.5)], rates uniform in +-4.03; mass scales in [0.6, 1.4] when asked.  (root [n,13], dof [n,33,2],
    mass_scale [n,38]) as float32."""
    r = np.random.default_rng(seed)
    root = np.zeros((n, 13))
    root[:, 0:2] = r.uniform(-xy, xy, (n, 2))
    root[:, 2] = r.uniform(0.5, 1.2, n)
    q = r.normal(size=(n, 4))
    root[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    root[:, 7:10] = r.normal(0.0, 1.0, (n, 3))
    root[:, 10:13] = r.normal(0.0, 2.0, (n, 3))
    lo, hi = np.maximum(np.asarray(MODEL.dof_lower), -1.5), np.minimum(np.asarray(MODEL.dof_upper), 1.5)
    dof = np.stack([r.uniform(lo, hi, (n, 33)), r.uniform(-4.03, 4.03, (n, 33))], -1)
    ms = r.uniform(0.6, 1.4, (n, NB)) if mass else np.ones((n, NB))
    return root.astype(F), dof.astype(F), ms.astype(F)


# ---------------------------------------------------------------------------------------------- the tolerance
@functools.lru_cache(maxsize=None)
def measured(vel_at_com):
    """d per channel: the float32 recursion against the float64 one at STATES seeded states."""
    root, dof, ms = states(STATES, 20260 + vel_at_com, mass=True)
    a, b = chain(root, dof, np.float64, vel_at_com), chain(root, dof, np.float32, vel_at_com)
    ra, rb = rows(a, vel_at_com), rows(b, vel_at_com)
    ca, cb = com(a, ms), com(b, ms)
    dev = lambda x, y: float(np.abs(x - y.astype(np.float64)).max())          # noqa: E731
    return {"off": dev(ra["off"], rb["off"]), "R": dev(ra["R"], rb["R"]), "qnorm": float(np.abs(np.linalg.norm(rb["q"].astype(np.float64), axis=-1) - 1).max()),
            "vel": dev(ra["vel"], rb["vel"]), "w": dev(ra["w"], rb["w"]), "com_off": dev(ca[0], cb[0]), "com_vel": dev(ca[1], cb[1]),
            "mass": dev(ca[2], cb[2])}


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, F))).astype(np.float64)


def excess(got_states, got_com, root, dof, ms, vel_at_com, ids=None, report=None):
    """Every channel of got_states [N,K,13] / got_com [N,7] (either may be None) against the float64 reference, as the largest deviation
    divided by its allowance (FACTOR * d; positions: + one ulp of |x|): a dict channel -> ratio; all must be <= 1."""
    d = measured(int(bool(vel_at_com)))
    c = chain(root, dof, np.float64, vel_at_com)
    base = np.asarray(root, F).astype(np.float64)[:, None, 0:3]
    out = {}
    if got_states is not None:
        g = np.asarray(got_states, F).astype(np.float64)
        r = rows(c, vel_at_com, ids)
        x = base + r["off"]
        out["pos"] = float((np.abs(g[..., 0:3] - x) / (FACTOR * d["off"] + ulp(x))).max())
        out["R"] = float(np.abs(qmat(g[..., 3:7]) - r["R"]).max() / (FACTOR * d["R"]))
        out["qnorm"] = float(np.abs(np.linalg.norm(g[..., 3:7], axis=-1) - 1).max() / (FACTOR * d["qnorm"]))
        out["vel"] = float(np.abs(g[..., 7:10] - r["vel"]).max() / (FACTOR * d["vel"]))
        out["w"] = float(np.abs(g[..., 10:13] - r["w"]).max() / (FACTOR * d["w"]))
    if got_com is not None:
        g = np.asarray(got_com, F).astype(np.float64)
        co, cv, cm = com(c, ms)
        x = base[:, 0] + co
        out["com_pos"] = float((np.abs(g[:, 0:3] - x) / (FACTOR * d["com_off"] + ulp(x))).max())
        out["com_vel"] = float(np.abs(g[:, 3:6] - cv).max() / (FACTOR * d["com_vel"]))
        out["mass"] = float(np.abs(g[:, 6] - cm).max() / (FACTOR * d["mass"]))
    if report is not None:
        print(report, {k: round(v, 3) for k, v in out.items()}, "d:", {k: "%.2e" % v for k, v in d.items()})
    return out


def within(ex: dict) -> bool:
    return all(np.isfinite(v) and v <= 1.0 for v in ex.values())
