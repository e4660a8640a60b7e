"""A numpy restatement of the gait profile's record (include/dyros_gait.h) and the seeded synthetic buffers the CPU and GPU tests share."""
import numpy as np

from isaacgymdyros_amd import abi
from isaacgymdyros_amd import gait_profile as G

K, E = G.K, abi.K
F = np.float32
W = K["DWG_W"]
LF, RF = 8, 16                     # DWS_LFOOT, DWS_RFOOT
EDGES = (0, 299, 300, 1499, 1500, 2099, 2100, 3299, 3300, 3598)
# the spans a NaN is put into in turn: (buffer, a function env -> index of a word that is read)
NAN_SPANS = {
    "sole_l": ("cf", lambda e: (e, LF, 2)), "sole_r": ("cf", lambda e: (e, RF, 2)), "total_mass": ("tm", lambda e: (e,)),
    "target_force": ("es", lambda e: (e, E["DW_ES_TARGET_FORCE"] + 1)), "root_z": ("root", lambda e: (e, 2)), "root_vx": ("root", lambda e: (e, 7)),
    "target_vel": ("es", lambda e: (e, E["DW_ES_TARGET_VEL"])), "dof_pos": ("dof", lambda e: (e, 11, 0)),
    "target_qpos": ("es", lambda e: (e, E["DW_ES_TARGET_QPOS"] + 5)), "action_torque": ("es", lambda e: (e, E["DW_ES_ACTION_TORQUE"] + 11)),
    "paid": ("stacked", lambda e: (e, K["DWG_PAID_COLUMN"])),
}
ORDER = ("root", "dof", "cf", "es", "stacked", "reset", "progress", "tm")          # dwg_record's buffer arguments, in its order


def fx(v):
    lim = float(1 << K["DWG_CLAMP_LOG2"])
    return np.rint(np.clip(np.asarray(v, np.float64), -lim, lim) * float(1 << K["DWG_FRAC_BITS"])).astype(np.int64)


class Synth:
    """Seeded buffers of n envs; step() gives fresh ones.  The mocap index is uniform over 0 .. 3598 with the window edges forced in (a
    different edge first on every step, so n = 1 meets several); sole forces are negative, exactly 1.0, and above the clamp in some envs."""

    def __init__(self, n, seed, nan_span=None, unread_nan=False):
        self.n, self.rng, self.t, self.nan_span, self.unread_nan = n, np.random.default_rng(seed), 0, nan_span, unread_nan

    def step(self):
        n, r = self.n, self.rng
        u = lambda *s: r.uniform(-1.0, 1.0, s).astype(F)          # noqa: E731
        root, dof = u(n, 13), u(n, E["DW_NUM_DOF"], 2)
        root[:, 2] += F(0.9)
        cf = (u(n, E["DW_NUM_BODIES"], 3) * F(40.0)).astype(F)
        cf[:, [LF, RF], 2] = r.uniform(-60.0, 1200.0, (n, 2)).astype(F) * (r.random((n, 2)) < 0.7)
        one = r.random((n, 2)) < 0.1
        cf[:, [LF, RF], 2] = np.where(one, F(1.0), cf[:, [LF, RF], 2])
        es = u(n, E["DW_ES_WORDS"])
        esi = es.view(np.int32)
        idx = r.integers(0, 3599, n)
        k = min(n, len(EDGES))
        idx[:k] = np.roll(EDGES, -self.t)[:k]
        esi[:, E["DW_ES_MOCAP_IDX"]] = idx
        esi[:, E["DW_ES_PERT_ON"]] = r.random(n) < 0.2
        es[:, E["DW_ES_TARGET_FORCE"]:E["DW_ES_TARGET_FORCE"] + 2] = -r.uniform(0.0, 1025.0, (n, 2)).astype(F)
        es[:, E["DW_ES_ACTION_TORQUE"]:E["DW_ES_ACTION_TORQUE"] + 12] *= F(300.0)
        stacked = u(n, 15)
        stacked[:, K["DWG_PAID_COLUMN"]] = r.choice(np.asarray([0.0, 0.2, -1.0], F), n)
        reset = (r.random(n) < 0.1).astype(np.int64) * r.integers(1, 3, n)
        progress = r.integers(0, 12, n).astype(np.int64)
        tm = r.uniform(90.0, 110.0, n).astype(F)
        if n > 12:
            cf[11, LF, 2], cf[12, RF, 2] = F(3.0e9), F(-3.0e9)          # (above the clamp; the square is clamped as well)
            es[11, E["DW_ES_ACTION_TORQUE"]] = F(2.0e9)
            reset[11:13], progress[11:13], esi[11:13, E["DW_ES_PERT_ON"]] = 0, 50, 0
        b = dict(root=root, dof=dof, cf=cf, es=es, stacked=stacked, reset=reset, progress=progress, tm=tm)
        if self.nan_span is not None:
            name, at = NAN_SPANS[self.nan_span]
            bad = [np.nan, np.inf, -np.inf]
            for i, e in enumerate(range(0, n, 3)):
                b[name][at(e)] = bad[i % 3]
        if self.unread_nan:          # words that are not read do not discard an env-step
            root[:, 0], dof[:, 20, 1], cf[:, 3, 0], es[:, E["DW_ES_TARGET_QPOS"] + 20], stacked[:, 0] = np.nan, np.nan, np.inf, np.nan, np.nan
        self.t += 1
        return tuple(np.ascontiguousarray(b[k]) for k in ORDER)


def record(bufs, bins, min_episode_step, skip_pushes, table, ct):
    """dwg_record on numpy buffers: table [bins, DWG_W] int64 and ct [DWG_CT_WORDS] int64 are added to."""
    root, dof, cf, es, stacked, reset, progress, tm = bufs
    esi = es.view(np.int32)
    idx, pert = esi[:, E["DW_ES_MOCAP_IDX"]], esi[:, E["DW_ES_PERT_ON"]] != 0
    fl, fr = cf[:, LF, 2], cf[:, RF, 2]
    tf = es[:, E["DW_ES_TARGET_FORCE"]:E["DW_ES_TARGET_FORCE"] + 2]
    tv0 = es[:, E["DW_ES_TARGET_VEL"]]
    q, tq = dof[:, :12, 0], es[:, E["DW_ES_TARGET_QPOS"]:E["DW_ES_TARGET_QPOS"] + 12]
    tau = es[:, E["DW_ES_ACTION_TORQUE"]:E["DW_ES_ACTION_TORQUE"] + 12]
    paid = stacked[:, K["DWG_PAID_COLUMN"]]
    terminal = reset != 0
    filtered = ~terminal & ((progress < min_episode_step) | (pert & bool(skip_pushes)))
    finite = (np.isfinite(np.column_stack([fl, fr, tm, tf, root[:, 2], root[:, 7], tv0, paid, q, tq, tau])).all(axis=1)
              & (idx >= 0) & (idx < K["DWG_ROWS"]))
    discarded = ~terminal & ~filtered & ~finite
    rec = ~terminal & ~filtered & finite
    ct += np.asarray([rec.sum(), terminal.sum(), filtered.sum(), discarded.sum()], np.int64)
    m = int(rec.sum())
    if m == 0:
        return
    fl, fr, tm, tf, tv0, q, tq, tau, paid, pert = fl[rec], fr[rec], tm[rec], tf[rec], tv0[rec], q[rec], tq[rec], tau[rec], paid[rec], pert[rec]
    width = K["DWG_ROWS"] // bins
    b = idx[rec] // width
    win = np.asarray([G.window_of(int(x) * width) for x in b])
    with np.errstate(over="ignore"):
        ws = tm / F(104.48)
        lcon, rcon = fl > F(1.0), fr > F(1.0)
        pay = np.where(win == K["DWG_WIN_DSP"], rcon & lcon, np.where(win == K["DWG_WIN_RSSP"], rcon & ~lcon, ~rcon & lcon))
        v = np.zeros((m, W), np.int64)
        v[:, 0] = 1
        v[:, 1], v[:, 2] = fx(fl), fx(fr)
        v[:, 3], v[:, 4] = fx(fl.astype(np.float64) ** 2), fx(fr.astype(np.float64) ** 2)
        v[:, 5], v[:, 6] = fx(-(ws * tf[:, 0])), fx(-(ws * tf[:, 1]))
        v[:, 7], v[:, 8] = fx(np.abs(fl + ws * tf[:, 0])), fx(np.abs(fr + ws * tf[:, 1]))
        v[:, 9], v[:, 10] = lcon, rcon
        v[:, 11], v[:, 12] = paid > F(0.0), pay
        v[:, 13], v[:, 14] = fx(root[rec, 2]), fx(root[rec, 7] - tv0)
        v[:, 15] = pert
        v[:, 16:28] = fx(np.abs(q - tq))
        v[:, 28:40] = fx(np.abs(tau))
    np.add.at(table, b, v)
