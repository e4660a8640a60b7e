"""The foot force-torque sensors restated in numpy (include/dyros_sensors.h), shared by tests/test_force_sensors.py
(the g++ build of csrc/dw_sensors.h) and tests/test_force_sensors_gpu.py (the HIP kernel).  Test helper, in the style of
tests/body_states_ref.py, whose chain() gives the foot pose.

compute(root, dof, warm, inv_dt, sensors, dtype) is the header's semantics in one number format: float64 is the reference, float32 the
measure of what the format costs.  Both are evaluated at the same float32 inputs (inv_dt, a float32 by definition, among them); the model's
corners and the sensors' mounts are the float64 values in the reference and their float32 roundings (what the argument block holds) in
float32, so d includes what rounding the constants costs.

The tolerance is measured here, against the reference and never against a kernel, with section 21's method: per channel, d = the largest
deviation of the float32 restatement from the float64 one over STATES seeded states, and what is tested must be within FACTOR * d.  A world
position is held to FACTOR * d_offset + one float32 ulp of |x| per coordinate (the base is added last, with one rounding).  Counts are
exact.
"""
import functools

import numpy as np

import body_states_ref as BR

MODEL = BR.MODEL
FACTOR, STATES = 4.0, 4096
F = np.float32
FOOT_MV = [MODEL.foot_pts[0]["moving"], MODEL.foot_pts[4]["moving"]]
FOOT_POS = np.asarray([p["pos"] for p in MODEL.foot_pts], np.float64)          # [8, 3]; corners 0..3 left, 4..7 right
DEFAULT_SENSORS = [{"foot": 0, "pos": [0.0, 0.0, -0.09], "quat": [0.0, 0.0, 0.0, 1.0], "world_frame": False},
                   {"foot": 1, "pos": [0.0, 0.0, -0.09], "quat": [0.0, 0.0, 0.0, 1.0], "world_frame": False}]
DT = 0.002
INV_DT = F(1.0) / F(DT)          # as the step forms it: 1.0f / (float)dt
FMAX = 1500.0          # N: the largest normal force on a corner in states() (a sole then carries up to six body weights, a landing)


def foot_poses(root, dof, dtype=np.float64):
    """(off [N,2,3] offset of each foot from the base, R [N,2,3,3]) in one number format."""
    c = BR.chain(root, dof, dtype)
    return c["off"][:, FOOT_MV], c["R"][:, FOOT_MV]


def compute(root, dof, warm, inv_dt=INV_DT, sensors=DEFAULT_SENSORS, dtype=np.float64):
    """dict of F [N,S,3], T [N,S,3] (the rows' two halves), cop [N,2,4], zmp_off [N,2] (offset from the base), zmp_fz [N], zmp_cnt [N],
    zmp_on [N] bool, cor_off [N,8,3], cor_f [N,8,3]; warm: [N,8,3] or [N,24] float32 impulses."""
    T = np.dtype(dtype).type
    root = np.asarray(root)
    N = len(root)
    off, R = foot_poses(root, dof, dtype)
    f = np.asarray(warm, F).reshape(N, 8, 3).astype(dtype) * T(F(inv_dt))          # f_k, world
    cpos = FOOT_POS.astype(dtype)
    out = {}
    Fs, Ts = np.zeros((N, len(sensors), 3), dtype), np.zeros((N, len(sensors), 3), dtype)
    for s, sen in enumerate(sensors):
        ft = int(sen["foot"])
        pos = np.asarray(sen.get("pos", [0, 0, -0.09]), np.float64).astype(dtype)
        q = np.asarray(sen.get("quat", [0, 0, 0, 1]), np.float64)
        q = (q if dtype == np.float64 else q.astype(F)).astype(dtype)          # (float32: the rounded quaternion, as the argument block holds it)
        Fw, Tw = np.zeros((N, 3), dtype), np.zeros((N, 3), dtype)
        for k in range(4 * ft, 4 * ft + 4):
            r = BR.mv3(R[:, ft], (cpos[k] - pos)[None, :])
            Fw = Fw + f[:, k]
            Tw = Tw + BR.cross(r, f[:, k])
        if not sen.get("world_frame", False):
            Rt = np.swapaxes(R[:, ft], -1, -2)
            Rs = BR.qmat(q[None, :])[0].T
            Fw, Tw = BR.mv3(Rs[None], BR.mv3(Rt, Fw)), BR.mv3(Rs[None], BR.mv3(Rt, Tw))
        Fs[:, s], Ts[:, s] = Fw, Tw
    out["F"], out["T"] = Fs, Ts
    n = f[:, :, 2]
    cop = np.zeros((N, 2, 4), dtype)
    for ft in range(2):
        sx, sy, sn, cnt = (np.zeros(N, dtype) for _ in range(4))
        for k in range(4 * ft, 4 * ft + 4):
            sx, sy, sn = sx + n[:, k] * cpos[k, 0], sy + n[:, k] * cpos[k, 1], sn + n[:, k]
            cnt = cnt + (n[:, k] > 0)
        on = sn > 0
        d = np.where(on, sn, T(1))
        cop[:, ft] = np.where(on[:, None], np.stack([sx / d, sy / d, sn, cnt], -1), T(0))
    out["cop"] = cop
    co = np.stack([off[:, k // 4] + BR.mv3(R[:, k // 4], cpos[k][None, :]) for k in range(8)], 1)          # [N,8,3]
    sx, sy, sn, cnt = (np.zeros(N, dtype) for _ in range(4))
    for k in range(8):
        sx, sy, sn = sx + n[:, k] * co[:, k, 0], sy + n[:, k] * co[:, k, 1], sn + n[:, k]
        cnt = cnt + (n[:, k] > 0)
    on = sn > 0
    d = np.where(on, sn, T(1))
    out["zmp_off"] = np.where(on[:, None], np.stack([sx / d, sy / d], -1), T(0))
    out["zmp_fz"], out["zmp_cnt"], out["zmp_on"] = np.where(on, sn, T(0)), np.where(on, cnt, T(0)), on
    out["cor_off"], out["cor_f"] = co, f
    return out


# ---------------------------------------------------------------------------------------------- inputs
def states(n, seed, xy=1.0):
    """Seeded inputs: body_states_ref.states' base attitudes and joint angles within limits, and impulses [n,8,3]: normal force uniform in
    [0, FMAX] N per corner, tangential within the mu = 1 cone, a third of the corners unloaded (exactly zero), one env in eight with a whole
    sole in the air and one in sixteen with both.  (root [n,13], dof [n,33,2], warm [n,8,3]) as float32."""
    root, dof, _ = BR.states(n, seed, xy=xy)
    r = np.random.default_rng(seed + 7919)
    fz = r.uniform(0.0, FMAX, (n, 8))
    fz[r.random((n, 8)) < 1.0 / 3.0] = 0.0
    air = r.integers(0, 16, n)
    fz[air == 1, 0:4] = 0.0
    fz[air == 2, 4:8] = 0.0
    fz[air == 3, :] = 0.0
    ang, mag = r.uniform(0, 2 * np.pi, (n, 8)), r.uniform(0, 1, (n, 8)) * fz
    f = np.stack([mag * np.cos(ang), mag * np.sin(ang), fz], -1)
    return root, dof, (f * DT).astype(F)


def sensors8():
    """Eight sensors with repeats, mixed world_frame and non-identity quaternions (unit, in double)."""
    r = np.random.default_rng(5)
    out = []
    for s in range(8):
        q = r.normal(size=4)
        q = q / np.linalg.norm(q)
        out.append({"foot": [0, 1, 1, 0, 0, 1, 0, 1][s], "pos": [0.0, 0.0, -0.09] if s < 2 else r.uniform(-0.1, 0.1, 3).tolist(),
                    "quat": [0.0, 0.0, 0.0, 1.0] if s in (0, 5) else q.tolist(), "world_frame": s in (2, 3, 5)})
    out[6] = dict(out[0])          # a repeat
    return out


# ---------------------------------------------------------------------------------------------- the tolerance
@functools.lru_cache(maxsize=None)
def measured():
    """d per channel: the float32 restatement against the float64 one at STATES seeded states, eight sensors."""
    root, dof, warm = states(STATES, 20262)
    S = sensors8()
    a, b = compute(root, dof, warm, INV_DT, S, np.float64), compute(root, dof, warm, INV_DT, S, np.float32)
    dev = lambda x, y: float(np.abs(x - y.astype(np.float64)).max())          # noqa: E731
    return {"force": max(dev(a["F"], b["F"]), dev(a["cor_f"], b["cor_f"]), dev(a["cop"][..., 2], b["cop"][..., 2]), dev(a["zmp_fz"], b["zmp_fz"])),
            "torque": dev(a["T"], b["T"]), "cop": dev(a["cop"][..., 0:2], b["cop"][..., 0:2]), "zmp_off": dev(a["zmp_off"], b["zmp_off"]),
            "cor_off": dev(a["cor_off"], b["cor_off"])}


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, F))).astype(np.float64)


def excess(got, root, dof, warm, inv_dt=INV_DT, sensors=DEFAULT_SENSORS, report=None):
    """got: dict with any of sensors [N,S,6], cop [N,2,4], zmp [N,4], corners [N,8,6] (None entries are skipped) against the float64
    reference, as the largest deviation divided by its allowance: a dict channel -> ratio; all must be <= 1.  Counts and the all-zero rows of
    unloaded soles must be exact (ratio inf otherwise)."""
    d = measured()
    ref = compute(root, dof, warm, inv_dt, sensors, np.float64)
    base = np.asarray(root, F).astype(np.float64)
    g = {k: None if v is None else np.asarray(v, F).astype(np.float64) for k, v in got.items()}
    bad = lambda ok: 0.0 if ok else float("inf")          # noqa: E731
    out = {}
    if g.get("sensors") is not None and len(sensors):
        out["force"] = float(np.abs(g["sensors"][..., 0:3] - ref["F"]).max() / (FACTOR * d["force"]))
        out["torque"] = float(np.abs(g["sensors"][..., 3:6] - ref["T"]).max() / (FACTOR * d["torque"]))
    if g.get("cop") is not None:
        out["cop"] = float(np.abs(g["cop"][..., 0:2] - ref["cop"][..., 0:2]).max() / (FACTOR * d["cop"]))
        out["cop_fz"] = float(np.abs(g["cop"][..., 2] - ref["cop"][..., 2]).max() / (FACTOR * d["force"]))
        out["cop_count"] = bad(np.array_equal(g["cop"][..., 3], ref["cop"][..., 3]) and not g["cop"][ref["cop"][..., 2] <= 0].any())
    if g.get("zmp") is not None:
        x = np.where(ref["zmp_on"][:, None], base[:, 0:2] + ref["zmp_off"], 0.0)
        out["zmp"] = float((np.abs(g["zmp"][:, 0:2] - x) / (FACTOR * d["zmp_off"] + ulp(x))).max())
        out["zmp_fz"] = float(np.abs(g["zmp"][:, 2] - ref["zmp_fz"]).max() / (FACTOR * d["force"]))
        out["zmp_count"] = bad(np.array_equal(g["zmp"][:, 3], ref["zmp_cnt"]) and not g["zmp"][~ref["zmp_on"]].any())
    if g.get("corners") is not None:
        x = base[:, None, 0:3] + ref["cor_off"]
        out["cor_pos"] = float((np.abs(g["corners"][..., 0:3] - x) / (FACTOR * d["cor_off"] + ulp(x))).max())
        out["cor_force"] = float(np.abs(g["corners"][..., 3:6] - ref["cor_f"]).max() / (FACTOR * d["force"]))
    if report is not None:
        print(report, {k: round(v, 3) for k, v in out.items()}, "d:", {k: "%.2e" % v for k, v in d.items()})
    return out


def within(ex: dict) -> bool:
    return len(ex) > 0 and all(np.isfinite(v) and v <= 1.0 for v in ex.values())


def env_state_of(warm, words=372, at=344, fill=None):
    """[n, words] float32 task records holding warm [n,8,3] at `at`; the other words `fill` (a generator: random, so that a read beside
    the block shows)."""
    n = len(warm)
    es = np.zeros((n, words), F) if fill is None else fill.normal(size=(n, words)).astype(F)
    es[:, at:at + 24] = np.asarray(warm, F).reshape(n, 24)
    return es


def step_force_tolerance(warm, inv_dt=INV_DT):
    """[N,2,3]: how far a foot's sum_k WARM[k] * inv_dt, formed in float32, may stand from the step's own row of contact_forces, which is
    (sum_k WARM[k]) * inv_dt in float32 over the same stored impulses.  With A = sum_k |f_k,i|: the step makes three additions and one
    product (each within half an ulp of A), this side four products (half an ulp of |f_k,i| each, together within half an ulp of A) and three
    additions: 4 ulp(A).  From the number format alone; the tests print the share of it they use."""
    f = np.abs(np.asarray(warm, F).reshape(len(warm), 2, 4, 3).astype(np.float64) * float(F(inv_dt)))
    return 4.0 * ulp(f.sum(2))
