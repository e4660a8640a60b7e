"""DyrosDynamicWalk's on-GPU gait profile (include/dyros_gait.h, csrc/dw_gait.hip): the gait binned by mocap phase.

Opt-in: cfg["sim"]["mi355"]["gait_profile"] = {"bins": 72, "min_episode_step": 0, "skip_pushes": False} (or True for these defaults) gives
the env a `gait_profile` attribute (None otherwise).  Every step() then makes one more launch, dwg_record, on the step's stream: every env's
sole forces, contacts, the force the mocap table expects, whether foot_contact_reward was paid, root height, velocity error and the leg
joints' tracking errors and torques are added to the row of the env's phase bin, bin = mocap_data_idx // (3600 // bins).  The sums are
64-bit integers (2^-16 units), so a summary is the same bits from run to run and between eager and replayed steps.  No host sync and no
allocation per step, so the launch sits inside a captured rollout graph like the step itself.

    record()         after a step (DyrosDynamicWalk.step calls it)
    reset_totals()   starts a new window
    summary()        the window since construction or the last reset_totals() as a dict: one reduction launch, one device-to-host copy
    save_npz(path), export_txt(dir)

Env-steps that end an episode are not added (`skipped_terminal`): the step kernel resets an env in the launch that ends its episode, so such a
row would mix the ended episode's forces and phase with the new episode's pose.  `min_episode_step` and `skip_pushes` leave out the first
steps of an episode and the steps under a push (`skipped_filter`); an env-step with a non-finite input is `discarded`.
"""
from __future__ import annotations

import os

import numpy as np

from . import cbind
from .recorders import Recorder

K = cbind.constants("dyros_gait.h", "dwg_")
EXPORTS = list(cbind.signatures("dyros_gait.h", "dwg_"))
BINS = (12, 24, 36, 72, 144)
W, ROWS, NJ = K["DWG_W"], K["DWG_ROWS"], K["DWG_LEG_JOINTS"]
SCALE = float(1 << K["DWG_FRAC_BITS"])
WINDOWS = ("DSP", "RSSP", "LSSP")          # (DWG_WIN_*: double support, right and left single support)
COUNTERS = ("recorded", "skipped_terminal", "skipped_filter", "discarded")
DEFAULTS = {"bins": K["DWG_BINS_DEFAULT"], "min_episode_step": 0, "skip_pushes": False}
MOCAP_FORCE_COLS = (34, 35)
# per-bin columns of export_txt, in this order (after bin, phase, window)
TXT_COLUMNS = (["count", "fz_l", "fz_r", "fz_std_l", "fz_std_r", "expected_fz_l", "expected_fz_r", "force_err_l", "force_err_r",
                "contact_fraction_l", "contact_fraction_r", "paid_fraction", "paid_predicted_fraction", "root_z", "vel_err", "push_fraction",
                "mocap_force_l", "mocap_force_r"] + ["joint_err_%d" % j for j in range(NJ)] + ["torque_abs_%d" % j for j in range(NJ)])


def declare(lib) -> dict:
    return cbind.declare(lib, "dyros_gait.h", "dwg_")


def window_of(idx: int) -> int:
    """The reward's window of mocap row idx (dw_oct_post.h: DSP, RSSP, LSSP) as an index into WINDOWS."""
    if 300 <= idx < 1500:
        return K["DWG_WIN_RSSP"]
    if 2100 <= idx < 3300:
        return K["DWG_WIN_LSSP"]
    return K["DWG_WIN_DSP"]


def check_bins(bins) -> int:
    if isinstance(bins, bool) or not isinstance(bins, int) or bins not in BINS:
        raise ValueError("sim.mi355.gait_profile.bins must be one of %s, got %r" % (list(BINS), bins))
    return bins


def bin_windows(bins: int) -> list:
    """The window index of every bin (every allowed bin lies in one window)."""
    width = ROWS // check_bins(bins)
    return [window_of(b * width) for b in range(bins)]


def resolve(spec) -> dict:
    """cfg sim.mi355.gait_profile as a full dict; None when the profile is off (None or False).  ValueError for anything else that is not
    True or a dict of bins / min_episode_step / skip_pushes in range."""
    if spec is None or spec is False:
        return None
    if spec is True:
        return dict(DEFAULTS)
    if not isinstance(spec, dict):
        raise ValueError("sim.mi355.gait_profile must be True, False or a dict with bins, min_episode_step and skip_pushes")
    unknown = set(spec) - set(DEFAULTS)
    if unknown:
        raise ValueError("sim.mi355.gait_profile: unknown keys %s" % sorted(unknown))
    out = dict(DEFAULTS, **spec)
    check_bins(out["bins"])
    m = out["min_episode_step"]
    if isinstance(m, bool) or not isinstance(m, int) or not 0 <= m < 2 ** 31:
        raise ValueError("sim.mi355.gait_profile.min_episode_step must be a non-negative integer, got %r" % (m,))
    if not isinstance(out["skip_pushes"], bool):
        raise ValueError("sim.mi355.gait_profile.skip_pushes must be True or False")
    return out


def validate(spec, num_envs=None) -> None:
    """Range checks of cfg sim.mi355.gait_profile (config.validate_cfg)."""
    resolve(spec)


def mocap_force(bins: int, mocap: np.ndarray = None) -> np.ndarray:
    """[bins, 2] the per-bin mean of the mocap table's two force columns (left, right), unscaled; mocap None: the packaged table."""
    if mocap is None:
        mocap = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets", "mocap_walk_f32.npy"))
    f = np.asarray(mocap, np.float64)[:ROWS, list(MOCAP_FORCE_COLS)]
    return f.reshape(check_bins(bins), ROWS // bins, 2).mean(axis=1)


def _means(t: np.ndarray) -> dict:
    """The derived means of table rows t [..., DWG_W] int64 (one per bin, or one window's sum), in float64; nan where count is 0."""
    t = np.asarray(t, np.int64)
    n = t[..., K["DWG_R_COUNT"]].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = lambda a, k: t[..., a:a + k].astype(np.float64) / SCALE / n[..., None]          # noqa: E731
        frac = lambda a, k: t[..., a:a + k].astype(np.float64) / n[..., None]                  # noqa: E731
        fz, fz2 = mean(K["DWG_R_FZ"], 2), mean(K["DWG_R_FZ2"], 2)
        return {"count": t[..., K["DWG_R_COUNT"]].copy(), "fz": fz, "fz_std": np.sqrt(np.maximum(fz2 - fz * fz, 0.0)),
                "expected_fz": mean(K["DWG_R_EXPECTED"], 2), "force_err": mean(K["DWG_R_FERR"], 2),
                "contact_fraction": frac(K["DWG_R_CONTACT"], 2), "paid_fraction": frac(K["DWG_R_PAID"], 1)[..., 0],
                "paid_predicted_fraction": frac(K["DWG_R_PREDICTED"], 1)[..., 0], "root_z": mean(K["DWG_R_ROOT_Z"], 1)[..., 0],
                "vel_err": mean(K["DWG_R_VEL_ERR"], 1)[..., 0], "push_fraction": frac(K["DWG_R_PERT"], 1)[..., 0],
                "joint_err": mean(K["DWG_R_JOINT_ERR"], NJ), "torque_abs": mean(K["DWG_R_TORQUE"], NJ)}


def fold(table: np.ndarray, ct, mocap: np.ndarray = None) -> dict:
    """The summary dict from the [bins, DWG_W] int64 table and the DWG_CT_WORDS counters."""
    table = np.asarray(table, np.int64)
    bins = check_bins(int(table.shape[0]))
    win = np.asarray(bin_windows(bins))
    out = _means(table)
    out["bins"] = bins
    out["phase"] = (np.arange(bins) + 0.5) / bins
    out["window"] = [WINDOWS[w] for w in win]
    out["mocap_force"] = mocap_force(bins, mocap)
    out["windows"] = {}
    for w, name in enumerate(WINDOWS):
        d = _means(table[win == w].sum(axis=0))
        d["count"] = int(d["count"])
        d["mocap_force"] = out["mocap_force"][win == w].mean(axis=0)
        out["windows"][name] = d
    tot = table.sum(axis=0)
    n = int(tot[K["DWG_R_COUNT"]])
    out["duty_factor"] = [int(tot[K["DWG_R_CONTACT"] + f]) / n if n else float("nan") for f in range(2)]
    for i, name in enumerate(COUNTERS):
        out[name] = int(ct[i])
    out["table"] = table
    return out


def flat(s: dict) -> dict:
    """A summary as save_npz writes it: arrays only (the windows as windows_<key> [3, ...] in WINDOWS' order)."""
    d = {k: np.asarray(v) for k, v in s.items() if k != "windows"}
    for k in s["windows"][WINDOWS[0]]:
        d["windows_" + k] = np.stack([np.asarray(s["windows"][w][k]) for w in WINDOWS])
    return d


def write_npz(path: str, s: dict):
    np.savez(path, **flat(s))


def _txt_row(s: dict, b: int) -> list:
    two = lambda k: [s[k][b][0], s[k][b][1]]          # noqa: E731
    return ([int(s["count"][b])] + two("fz") + two("fz_std") + two("expected_fz") + two("force_err") + two("contact_fraction")
            + [s[k][b] for k in ("paid_fraction", "paid_predicted_fraction", "root_z", "vel_err", "push_fraction")] + two("mocap_force")
            + list(s["joint_err"][b]) + list(s["torque_abs"][b]))


def write_txt(directory: str, s: dict) -> str:
    """gait_profile.txt: a header line, then one tab-separated line per bin (bin, phase, window, TXT_COLUMNS).  Returns the path."""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, "gait_profile.txt")
    with open(path, "w") as f:
        f.write("\t".join(["bin", "phase", "window"] + TXT_COLUMNS) + "\n")
        for b in range(s["bins"]):
            f.write("\t".join([str(b), repr(float(s["phase"][b])), s["window"][b]] + [repr(x if isinstance(x, int) else float(x)) for x in _txt_row(s, b)]) + "\n")
    return path


def read_txt(path: str) -> dict:
    """write_txt's file back: column name -> list (bin and count as int, window as str, the rest float)."""
    with open(path) as f:
        names = f.readline().rstrip("\n").split("\t")
        rows = [line.rstrip("\n").split("\t") for line in f]
    conv = lambda n: int if n in ("bin", "count") else (str if n == "window" else float)          # noqa: E731
    return {n: [conv(n)(r[i]) for r in rows] for i, n in enumerate(names)}


def format_table(s: dict) -> str:
    """The three-window table: the mean vertical sole force per foot beside the mocap force columns, and how often foot_contact_reward is
    paid (examples/ppo_player.py --gait-report)."""
    L = ["gait profile: %d env-steps in %d bins (%d terminal, %d filtered, %d discarded); duty factor L %.3f  R %.3f" % (
        s["recorded"], s["bins"], s["skipped_terminal"], s["skipped_filter"], s["discarded"], s["duty_factor"][0], s["duty_factor"][1]),
         "  %-5s %10s %9s %9s %11s %11s %9s %9s %8s %8s %7s %7s" % ("", "env-steps", "F_z L", "F_z R", "expected L", "expected R", "mocap L", "mocap R",
                                                                  "|err| L", "|err| R", "paid", "rule")]
    for name in WINDOWS:
        w = s["windows"][name]
        L.append("  %-5s %10d %9.1f %9.1f %11.1f %11.1f %9.1f %9.1f %8.1f %8.1f %7.3f %7.3f" % (
            name, w["count"], w["fz"][0], w["fz"][1], w["expected_fz"][0], w["expected_fz"][1], w["mocap_force"][0], w["mocap_force"][1],
            w["force_err"][0], w["force_err"][1], w["paid_fraction"], w["paid_predicted_fraction"]))
    return "\n".join(L)


def format_line(s: dict) -> str:
    """One log line: the paid fraction and the force error (left, right) per window."""
    return "gait: " + "  ".join("%s paid %.3f |F err| %.1f %.1f" % (n, w["paid_fraction"], w["force_err"][0], w["force_err"][1])
                                for n, w in s["windows"].items()) + "  (%d env-steps)" % s["recorded"]


class GaitProfile(Recorder):
    """The gait profile of one DyrosDynamicWalk env (see the module docstring).  Buffers are allocated here, once."""

    def __init__(self, env, spec=True):
        import torch
        spec = resolve(spec)
        if spec is None:
            raise ValueError("GaitProfile: the spec switches the profile off")
        super().__init__(env, declare)
        N, dev = self.num_envs, self._tdev
        self.bins = spec["bins"]
        self.min_episode_step, self.skip_pushes = spec["min_episode_step"], spec["skip_pushes"]
        self.groups = self.api["groups"](N)
        if self.groups < 0:
            raise ValueError("GaitProfile: num_envs %r is out of range" % (N,))
        self.part = torch.zeros(self.groups, self.bins, W, dtype=torch.int64, device=dev)
        self.ct = torch.zeros(K["DWG_CT_WORDS"], dtype=torch.int64, device=dev)
        self.out = torch.zeros(self.bins * W + K["DWG_CT_WORDS"], dtype=torch.int64, device=dev)
        p, f, i64 = self._in, torch.float32, torch.int64
        self._record_args = (
            N, self.bins, self.min_episode_step, int(self.skip_pushes), p("root_states", f, shape=(N, 13)), p("dof_state", f, numel=N * 66),
            p("contact_forces", f, shape=(N, env.num_bodies, 3)), p("env_state", f, numel=N * env._buf["env_state"].shape[1]),
            p("stacked_rewards", f, shape=(N, 15)), p("reset_buf", i64, shape=(N,)), p("progress_buf", i64, shape=(N,)),
            p("total_mass", f, numel=N), self.part.data_ptr(), self.ct.data_ptr())

    def record(self):
        """After a step, on the step's stream (DyrosDynamicWalk.step calls it)."""
        self._launch("record", self._record_args)

    def reset_totals(self):
        """Starts a new window."""
        self._launch("clear", (self.num_envs, self.bins, self.part.data_ptr(), self.ct.data_ptr()))

    def raw(self):
        """(table [bins, DWG_W] int64, counters [DWG_CT_WORDS] int64) as numpy arrays: one launch, one device-to-host copy."""
        self._launch("summarize", (self.num_envs, self.bins, self.part.data_ptr(), self.ct.data_ptr(), self.out.data_ptr()))
        o = self.out.cpu().numpy()
        return o[:self.bins * W].reshape(self.bins, W).copy(), o[self.bins * W:].copy()

    def summary(self) -> dict:
        return fold(*self.raw())

    def save_npz(self, path: str):
        write_npz(path, self.summary())

    def export_txt(self, directory: str) -> str:
        return write_txt(directory, self.summary())
