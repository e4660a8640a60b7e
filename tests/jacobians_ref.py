"""The Jacobian and mass-matrix tensors restated in numpy from the rules of include/dyros_jacobians.h, on top of
tests/body_states_ref.py's chain; shared by tests/test_jacobians.py (the g++ build of csrc/dw_jacobian.h) and tests/test_jacobians_gpu.py (the HIP
kernels).  Test helper.

The restatement is the header's DEFINITION, dense: a [6, 39] Jacobian at every point, and M = sum_k w_k Jlin' Jlin + Jang' (s R I R') Jang over 36
dense Jacobians at the records' COMs -- not the composite-body sums the kernels run, so agreement is a check of the algorithm as well.  Float64
is the reference; float32 (the model constants rounded as the device table rounds them) measures what the format costs.

The tolerance is measured here, against the reference and never against a kernel (tests/body_states_ref.py's method): per channel, d = the
largest deviation of the float32 restatement from the float64 one over STATES seeded states(..., mass=True), and what is tested must be within
FACTOR * d.  Channels: J's linear entries (columns 3:39 of rows 0:3; the rest of the base block is exact), J's angular entries, M's base-base,
base-joint and joint-joint blocks, and the COM Jacobian.
"""
import functools

import numpy as np

import body_states_ref as R

NB, NM, NI, NV = R.NB, R.NM, R.NI, 39
FACTOR, STATES = R.FACTOR, R.STATES
F = np.float32
INERT_I = np.asarray(R.MODEL.inert_I, np.float64)          # [36, 3, 3], the carrier's frame

# moving body m -> the moving bodies b >= 1 that are m or its ancestors, base side first
ANC = []
for _m in range(NM):
    _p, _b = [], _m
    while _b > 0:
        _p.append(_b)
        _b = R.MV_PARENT[_b]
    ANC.append(_p[::-1])


def dof_mask(ids=None):
    """[K, 39] bool: the columns of a row that can be non-zero."""
    ids = list(range(NB)) if ids is None else list(ids)
    m = np.zeros((len(ids), NV), bool)
    m[:, 0:6] = True
    for r, g in enumerate(ids):
        m[r, [5 + b for b in ANC[R.CARRIER[g]]]] = True
    return m


def branch_mask():
    """[39, 39] bool: the entries of M that can be non-zero (the base with everything; two joints when one is the other's ancestor)."""
    m = np.zeros((NV, NV), bool)
    m[0:6, :] = m[:, 0:6] = True
    for i in range(1, NM):
        for j in ANC[i]:
            m[5 + i, 5 + j] = m[5 + j, 5 + i] = True
    return m


def skew(v):
    z = np.zeros_like(v[..., 0])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1), np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def p_ref(c, vel_at_com):
    """The point whose velocity the root row holds, as an offset from the base [N, 3]."""
    dt = c["off"].dtype
    if not vel_at_com:
        return np.zeros((len(c["off"]), 3), dt)
    return R.mv3(c["R"][:, 0], R.INERT_COM[R.RECORD[0]].astype(dt))


def axes(c):
    """World joint axes a_b = R_b axis_b [N, 34, 3] (row 0 unused)."""
    dt = c["off"].dtype
    a = np.zeros_like(c["off"])
    for b in range(1, NM):
        a[:, b] = R.mv3(c["R"][:, b], R.MV_AXIS[b].astype(dt))
    return a


def jac_at(c, carriers, p, vel_at_com, a=None):
    """Dense Jacobians [N, K, 6, 39] at points p [N, K, 3] (offsets from the base) carried by moving bodies carriers [K]."""
    dt = c["off"].dtype
    N, K = p.shape[0], len(carriers)
    a = axes(c) if a is None else a
    J = np.zeros((N, K, 6, NV), dt)
    J[:, :, 0, 0] = J[:, :, 1, 1] = J[:, :, 2, 2] = J[:, :, 3, 3] = J[:, :, 4, 4] = J[:, :, 5, 5] = 1
    J[:, :, 0:3, 3:6] = -skew(p - p_ref(c, vel_at_com)[:, None])
    for r, m in enumerate(carriers):
        for b in ANC[m]:
            J[:, r, 0:3, 5 + b] = R.cross(a[:, b], p[:, r] - c["off"][:, b])
            J[:, r, 3:6, 5 + b] = a[:, b]
    return J


def points(c, vel_at_com, ids=None):
    """(carriers [K], points [N, K, 3]) of the rows of Gym bodies ids: the point whose velocity body_states_ref.rows reports."""
    dt = c["off"].dtype
    ids = list(range(NB)) if ids is None else list(ids)
    m = [R.CARRIER[g] for g in ids]
    p = c["off"][:, m].copy()
    if vel_at_com:
        for r, g in enumerate(ids):
            if R.RECORD[g] >= 0:
                p[:, r] = p[:, r] + R.mv3(c["R"][:, m[r]], R.INERT_COM[R.RECORD[g]].astype(dt))
    return m, p


def jacobian(c, vel_at_com, ids=None):
    """[N, K, 6, 39] of chain c."""
    m, p = points(c, vel_at_com, ids)
    J = jac_at(c, m, p, vel_at_com)
    for r, g in enumerate(range(NB) if ids is None else ids):
        if g == 0:          # exactly [I 0; 0 I | 0]
            J[:, r, 0:3, 3:6] = 0
    return J


def records(c, mass_scale=None):
    """(w [N, 36], COM offsets [N, 36, 3], s R I R' [N, 36, 3, 3]) of the inertial records."""
    dt = c["off"].dtype
    N = len(c["off"])
    ms = np.ones((N, NB), dt) if mass_scale is None else np.asarray(mass_scale, F).astype(dt)
    s = ms[:, R.INERT_GYM]
    w = R.INERT_MASS.astype(dt)[None, :] * s
    Rm = c["R"][:, R.INERT_MV]
    pc = c["off"][:, R.INERT_MV] + np.stack([R.mv3(Rm[:, k], R.INERT_COM[k].astype(dt)) for k in range(NI)], 1)
    Iw = s[:, :, None, None] * (Rm @ INERT_I.astype(dt)[None] @ np.swapaxes(Rm, -1, -2))
    return w, pc, Iw


def mass_matrix(c, vel_at_com, mass_scale=None, armature=None):
    """(M [N, 39, 39], sum_k w_k [N]) of chain c, the dense definition, a record at a time."""
    dt = c["off"].dtype
    w, pc, Iw = records(c, mass_scale)
    a = axes(c)
    M = np.zeros((len(w), NV, NV), dt)
    for k in range(NI):
        J = jac_at(c, [R.INERT_MV[k]], pc[:, k:k + 1], vel_at_com, a)[:, 0]
        Jl, Ja = J[:, 0:3], J[:, 3:6]
        M += w[:, k, None, None] * (np.swapaxes(Jl, -1, -2) @ Jl) + np.swapaxes(Ja, -1, -2) @ Iw[:, k] @ Ja
    if armature is not None:
        j = np.arange(33)
        M[:, 6 + j, 6 + j] += np.asarray(armature, F).astype(dt)
    return M, w.sum(-1, dtype=dt)


def nu(root, dof):
    """The generalised velocity [N, 39] in float64 of float32 states."""
    return np.concatenate([np.asarray(root, np.float64)[:, 7:13], np.asarray(dof, np.float64).reshape(len(root), 33, 2)[..., 1]], 1)


def kinetic_energy(c, vel_at_com, mass_scale=None):
    """sum_k (w v_c^2 + w' (s R I R') w) / 2 [N], from the chain's own velocities (no Jacobian)."""
    w, pc, Iw = records(c, mass_scale)
    om = c["w"][:, R.INERT_MV]
    vc = c["vo"][:, R.INERT_MV] + R.cross(om, pc - c["off"][:, R.INERT_MV])
    return 0.5 * (w * (vc * vc).sum(-1)).sum(-1) + 0.5 * np.einsum("nki,nkij,nkj->n", om, Iw, om)


# ---------------------------------------------------------------------------------------------- the tolerance
def armature_of(n, seed):
    """Seeded per-env armatures [n, 33] float32: the task's nominal values times uniform [0.8, 1.2]."""
    from isaacgymdyros_amd.task_constants import ARMATURE as NOMINAL
    return (np.asarray(NOMINAL, np.float64)[None, :] * np.random.default_rng(seed).uniform(0.8, 1.2, (n, 33))).astype(F)


CHANNELS = ("J_lin", "J_ang", "M_bb", "M_bj", "M_jj", "com_jac")


def split(J=None, M=None, CJ=None):
    """The channels of the outputs as a dict of arrays."""
    out = {}
    if J is not None:
        out["J_lin"], out["J_ang"] = J[..., 0:3, :], J[..., 3:6, :]
    if M is not None:
        out["M_bb"], out["M_bj"], out["M_jj"] = M[..., 0:6, 0:6], M[..., 0:6, 6:], M[..., 6:, 6:]
        out["M_jb"] = M[..., 6:, 0:6]
    if CJ is not None:
        out["com_jac"] = CJ
    return out


@functools.lru_cache(maxsize=None)
def measured(vel_at_com):
    """d per channel: the float32 restatement against the float64 one at STATES seeded states."""
    root, dof, ms = R.states(STATES, 23000 + vel_at_com, mass=True)
    arm = armature_of(STATES, 23002)
    d = {}
    pair = []
    for dt in (np.float64, np.float32):
        c = R.chain(root, dof, dt, vel_at_com)
        M, tot = mass_matrix(c, vel_at_com, ms, arm)
        pair.append(split(jacobian(c, vel_at_com), M, M[:, 0:3, :] / tot[:, None, None]))
    for ch in CHANNELS:
        d[ch] = float(np.abs(pair[0][ch] - pair[1][ch].astype(np.float64)).max())
    return d


def allowance(vel_at_com):
    """[39, 39] of FACTOR * d per entry of M."""
    d = measured(int(bool(vel_at_com)))
    A = np.full((NV, NV), FACTOR * d["M_bj"])
    A[0:6, 0:6] = FACTOR * d["M_bb"]
    A[6:, 6:] = FACTOR * d["M_jj"]
    return A


def excess(root, dof, ms, arm, vel_at_com, J=None, M=None, CJ=None, ids=None, report=None):
    """Every channel of the outputs given against the float64 reference, as the largest deviation divided by FACTOR * d: a dict channel ->
    ratio; all must be <= 1."""
    d = measured(int(bool(vel_at_com)))
    c = R.chain(root, dof, np.float64, vel_at_com)
    want = {}
    if J is not None:
        want.update(split(J=jacobian(c, vel_at_com, ids)))
    if M is not None or CJ is not None:
        Mr, tot = mass_matrix(c, vel_at_com, ms, arm)
        if M is not None:
            want.update(split(M=Mr))
        if CJ is not None:
            want["com_jac"] = Mr[:, 0:3, :] / tot[:, None, None]          # (the armature sits on the joints' diagonal: not in rows 0:3)
    got = split(None if J is None else np.asarray(J, F).astype(np.float64), None if M is None else np.asarray(M, F).astype(np.float64),
                None if CJ is None else np.asarray(CJ, F).astype(np.float64))
    out = {ch: float(np.abs(got[ch] - want[ch]).max() / (FACTOR * d["M_bj" if ch == "M_jb" else ch])) for ch in want}
    if report is not None:
        print(report, {k: round(v, 3) for k, v in out.items()}, "d:", {k: "%.2e" % v for k, v in d.items()})
    return out


def within(ex: dict) -> bool:
    return len(ex) > 0 and all(np.isfinite(v) and v <= 1.0 for v in ex.values())
