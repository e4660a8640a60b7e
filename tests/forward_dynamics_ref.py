"""The forward dynamics restated in numpy from the rules of include/dyros_forward_dynamics.h, on top of
tests/jacobians_ref.py's dense mass matrix; shared by tests/test_forward_dynamics.py (the g++ build of csrc/dw_factor.h) and
tests/test_forward_dynamics_gpu.py (the HIP kernel).  Test helper.

The reference is float64: np.linalg.solve and np.linalg.inv of jacobians_ref.mass_matrix for x and minv, and for the factor a plain-loop
M = L' D L (rows 38 down to 1, Featherstone's LTDL) restricted to the tree's pattern, which is derived here from the model's mv_parent.

The tolerance is measured here, against the reference and never against a kernel (tests/body_states_ref.py's method): per channel, d = the
largest deviation of the float32 run of the whole pipeline (the chain, M, the LTDL, both sweeps) from the float64 one over STATES seeded
states (dynamics_ref.seeded), and what is tested must be within FACTOR * d.  The right-hand sides are M64 accel_of(...) rounded to float32, so
that the solutions have the size of real accelerations.  Channels: x's base-linear, base-angular and joint words; minv's base-base,
base-joint and joint-joint blocks; the factor's D and L.
"""
import functools

import numpy as np

import body_states_ref as R
import dynamics_ref as DR
import jacobians_ref as JR

NV, NM = 39, R.NM
FACTOR, STATES = R.FACTOR, R.STATES
F = np.float32
U = 2.0 ** -24
CHANNELS = ("x_lin", "x_ang", "x_joint", "minv_bb", "minv_bj", "minv_jj", "factor_D", "factor_L")


def gamma(n):
    return n * U / (1 - n * U)


# ---------------------------------------------------------------------------------------------- the pattern, from mv_parent
ROWS = []
for _r in range(NV):
    _c = list(range(min(_r, 6)))
    if _r >= 6:
        _c += [5 + b for b in JR.ANC[_r - 5][:-1]]
    ROWS.append(_c + [_r])
PATTERN = sum(len(c) for c in ROWS)
ROW_START = np.concatenate([[0], np.cumsum([len(c) for c in ROWS])]).astype(np.int64)
COLS = np.array([(r << 8) | c for r in range(NV) for c in ROWS[r]], np.int64)
TCOLS = np.array([(r << 16) | int(ROW_START[r] + ROWS[r].index(c)) for c in range(NV) for r in range(c + 1, NV) if c in ROWS[r]], np.int64)
TCOL_START = np.concatenate([[0], np.cumsum([sum(1 for r in range(c + 1, NV) if c in ROWS[r]) for c in range(NV)])]).astype(np.int64)
MASK = np.zeros((NV, NV), bool)
for _r in range(NV):
    MASK[_r, ROWS[_r]] = True


def ltdl(M):
    """(L [N, 39, 39] unit lower triangular, D [N, 39]) with M = L' D L, in M's number format, by plain loops over the pattern."""
    H = np.array(M, copy=True)
    for k in range(NV - 1, 0, -1):
        cols = ROWS[k][:-1]
        for i in reversed(cols):          # (towards the base: row k's words at and below i are still M's when i is eliminated)
            a = H[:, k, i] / H[:, k, k]
            for j in cols:
                if j <= i:
                    H[:, i, j] = H[:, i, j] - a * H[:, k, j]
            H[:, k, i] = a
    D = H[:, np.arange(NV), np.arange(NV)].copy()
    L = np.tril(H, -1) * MASK[None]
    L[:, np.arange(NV), np.arange(NV)] = 1
    return L.astype(M.dtype), D


def solve(L, D, b):
    """M^-1 b for b [N, R, 39] by the two sweeps over the pattern, in L's number format."""
    b = np.array(b, dtype=L.dtype, copy=True)
    for k in range(NV - 1, 0, -1):
        for i in ROWS[k][:-1]:
            b[:, :, i] = b[:, :, i] - L[:, k, i, None] * b[:, :, k]
    b = b / D[:, None, :]
    for k in range(1, NV):
        v = b[:, :, k]
        for i in ROWS[k][:-1]:
            v = v - L[:, k, i, None] * b[:, :, i]
        b[:, :, k] = v
    return b


def factor_of(L, D):
    """The factor output's layout: D on the diagonal, L strictly below, zero elsewhere."""
    Fm = np.tril(L, -1)
    Fm[:, np.arange(NV), np.arange(NV)] = D
    return Fm


def mass_matrix(root, dof, vel_at_com, ms=None, arm=None, dtype=np.float64):
    return JR.mass_matrix(R.chain(root, dof, dtype, vel_at_com), vel_at_com, ms, arm)[0]


def pipeline(root, dof, vel_at_com, ms, arm, rhs=None, sub=None, dtype=np.float32):
    """dict of x [N, R, 39] (when rhs is given), minv and factor [N, 39, 39] in one number format, the way the kernel runs: the chain, M, the
    LTDL on the pattern, the sweeps; minv from the identity's columns, rows >= columns mirrored."""
    M = mass_matrix(root, dof, vel_at_com, ms, arm, dtype)
    L, D = ltdl(M)
    out = {"factor": factor_of(L, D)}
    X = solve(L, D, np.broadcast_to(np.eye(NV, dtype=dtype), (len(M), NV, NV)))          # X[:, c] = column c
    lower = np.tril(np.swapaxes(X, 1, 2))
    out["minv"] = lower + np.swapaxes(np.tril(lower, -1), 1, 2)
    if rhs is not None:
        b = np.asarray(rhs, F).astype(dtype)
        if sub is not None:
            b = b - np.asarray(sub, F).astype(dtype)[:, None, :]
        out["x"] = solve(L, D, b)
    return out


def evaluate(root, dof, vel_at_com, ms, arm, rhs=None, sub=None):
    """The float64 reference: x and minv by np.linalg.solve and inv of the dense mass matrix, the factor by the plain-loop LTDL."""
    M = mass_matrix(root, dof, vel_at_com, ms, arm)
    L, D = ltdl(M)
    out = {"factor": factor_of(L, D), "minv": np.linalg.inv(M), "M": M}
    if rhs is not None:
        b = np.asarray(rhs, F).astype(np.float64)
        if sub is not None:
            b = b - np.asarray(sub, F).astype(np.float64)[:, None, :]
        out["x"] = np.swapaxes(np.linalg.solve(M, np.swapaxes(b, 1, 2)), 1, 2)
    return out


def rhs_of(root, dof, vel_at_com, ms, arm, nrhs, seed):
    """Seeded right-hand sides [N, nrhs, 39] float32: M64 times seeded accelerations."""
    M = mass_matrix(root, dof, vel_at_com, ms, arm)
    a = np.stack([DR.accel_of(len(M), seed + r) for r in range(nrhs)], 1).astype(np.float64)
    return np.einsum("nab,nrb->nra", M, a).astype(F)


def split(out):
    ch = {}
    if out.get("x") is not None:
        ch["x_lin"], ch["x_ang"], ch["x_joint"] = out["x"][..., 0:3], out["x"][..., 3:6], out["x"][..., 6:]
    if out.get("minv") is not None:
        m = out["minv"]
        ch["minv_bb"], ch["minv_bj"], ch["minv_jj"] = m[..., 0:6, 0:6], np.concatenate([m[..., 0:6, 6:], np.swapaxes(m[..., 6:, 0:6], -1, -2)], -1), m[..., 6:, 6:]
    if out.get("factor") is not None:
        f = out["factor"]
        i = np.arange(NV)
        ch["factor_D"], ch["factor_L"] = f[..., i, i], f - f[..., i, i][..., None] * np.eye(NV)
    return ch


@functools.lru_cache(maxsize=None)
def measured(vel_at_com, plain=False):
    """d per channel: the float32 run of the pipeline against the float64 reference at STATES seeded states.  plain: the same states with nominal
    masses and no armature -- another matrix, whose condition number is seven times larger (2e5 against 3e4), so it has a d of its own."""
    root, dof, ms, arm, _acc = DR.seeded(STATES, 25000 + 10 * vel_at_com)
    if plain:
        ms = arm = None
    rhs = rhs_of(root, dof, vel_at_com, ms, arm, 1, 25005)
    a, b = split(evaluate(root, dof, vel_at_com, ms, arm, rhs)), split(pipeline(root, dof, vel_at_com, ms, arm, rhs))
    d = {ch: float(np.abs(a[ch] - b[ch].astype(np.float64)).max()) for ch in CHANNELS}
    d["x_scale"] = float(max(np.abs(a[ch]).max() for ch in ("x_lin", "x_ang", "x_joint")))          # the largest solution word d was measured with
    return d


def excess(got, root, dof, ms, arm, vel_at_com, rhs=None, sub=None, report=None, want=None):
    """Every channel of the outputs in dict `got` (x, minv, factor; any subset) against the float64 reference, as the largest deviation divided
    by FACTOR * d: a dict channel -> ratio; all must be <= 1.  ms and arm both None: the d of measured(..., plain=True)."""
    d = measured(int(bool(vel_at_com)), ms is None and arm is None)
    want = split(evaluate(root, dof, vel_at_com, ms, arm, rhs, sub) if want is None else want)
    have = split({k: None if v is None else np.asarray(v, F).astype(np.float64) for k, v in got.items()})
    out = {ch: float(np.abs(have[ch] - want[ch]).max() / (FACTOR * d[ch])) for ch in have}
    if report is not None:
        print(report, {k: round(v, 3) for k, v in out.items()}, "d:", {k: "%.2e" % v for k, v in d.items()})
    return out


def x_allowance(x_want, vel_at_com):
    """FACTOR * d per word of solutions x_want [..., 39] of any size: the solve is linear in the right-hand side, so its error grows with the
    solution; d was measured with solutions of up to d["x_scale"], and an env whose largest word is s times that gets s d."""
    d = measured(int(bool(vel_at_com)))
    own = np.array([d["x_lin"]] * 3 + [d["x_ang"]] * 3 + [d["x_joint"]] * 33)
    s = np.maximum(1.0, np.abs(x_want).max(-1, keepdims=True) / d["x_scale"])
    return FACTOR * own * s


def within(ex: dict) -> bool:
    return len(ex) > 0 and all(np.isfinite(v) and v <= 1.0 for v in ex.values())


def backward_error(factor, M):
    """The largest |L' D L - M|_ij / (2 gamma_18 (|L'| |D| |L|)_ij) over the lower triangle's pattern, the product formed in float64 from a
    float32 factor output, M the float32 mass matrix it factors.  The standard backward-error bound of a row of 17 entries, with a factor of
    two for the division; must be <= 1."""
    f = np.asarray(factor, F).astype(np.float64)
    i = np.arange(NV)
    D = f[:, i, i]
    L = np.tril(f, -1)
    L[:, i, i] = 1
    rec = np.einsum("nki,nk,nkj->nij", L, D, L)
    bound = 2 * gamma(18) * np.einsum("nki,nk,nkj->nij", np.abs(L), np.abs(D), np.abs(L))
    err = np.abs(rec - np.asarray(M, F).astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)          # (a word that is exact needs no allowance, even one of zero)
    return float(ratio[:, MASK | MASK.T].max())
