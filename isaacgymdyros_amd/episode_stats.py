"""DyrosDynamicWalk's on-GPU episode statistics (include/dyros_stats.h, csrc/dw_stats.hip).

Opt-in: cfg["sim"]["mi355"]["episode_stats"] = True gives the env an `episode_stats` attribute (None otherwise).  Every step() then
makes one more launch, dws_record, on the step's stream: why each finished episode ended (`extras["termination_cause"]`, a uint8 [N]
buffer overwritten in place), and sums of per-episode quantities folded into a window.  No host sync and no allocation per step, so
the launch sits inside a captured rollout graph like the step itself.

    summary()        the window since construction or the last reset_totals(), as a dict: one reduction launch and one device-to-host
                     copy
    reset_totals()   starts a new window (running episodes keep their counters)
    CAUSES           cause code -> name

Explicit reset_idx(), load_state_dict() and construction discard the running episode of the envs they touch (dws_restart): it is not
counted, and the per-env counters restart from progress_buf.
"""
from __future__ import annotations

import torch

from . import cbind
from .ppo_update import _req
from .recorders import EpisodeWindow, Window, div

K = cbind.constants("dyros_stats.h", "dws_")
K["DWS_SUM_AC"] = K["DWS_CT_WORDS"]                                  # (defined by expression in the header)
K["DWS_SUM_WORDS"] = K["DWS_CT_WORDS"] + K["DWS_AC_WORDS"]
EXPORTS = list(cbind.signatures("dyros_stats.h", "dws_"))
CAUSES = {0: "none", 1: "time_limit", 2: "non_foot_contact", 3: "orientation", 4: "non_finite"}
CMD_EDGES = (0.0, 0.2, 0.4, 0.6, 0.8)


def declare(lib) -> dict:
    return cbind.declare(lib, "dyros_stats.h", "dws_")


def validate(spec, num_envs=None) -> None:
    """cfg sim.mi355.episode_stats (config.validate_cfg): a bool."""
    if not isinstance(spec, bool):
        raise ValueError("sim.mi355.episode_stats must be True or False")


def fold(out, num_envs: int, max_episode_length: float, body_names) -> dict:
    """The summary dict from dws_summarize's [DWS_SUM_WORDS] doubles (a sequence of Python floats)."""
    w = Window(out, K, "DWS_")
    ct, ac = w.ct, w.ac
    s = w.head({CAUSES[c]: ct("CAUSE", c) for c in range(1, 5)}, body_names, max_episode_length)
    eps, env_steps = s["episodes"], s["records"] * num_envs
    bins = []
    for b in range(K["DWS_CMD_BINS"]):
        ne, nr, nq = ct("BIN_EP", b), ct("BIN_ROOT", b), ct("BIN_RATIO", b)
        bins.append(dict(lo=CMD_EDGES[b], hi=CMD_EDGES[b + 1], episodes=ne, vel_error=div(ac("VERR", b), nr),
                         lateral_drift=div(ac("DRIFT", b), nr), distance_ratio=div(ac("RATIO", b), nq), ratio_episodes=nq))
    gate_at = ct("GATE_AT")
    s.update(
        command_bins=bins,
        sole_over_1400=[div(ct("PK_OVER", f), eps) for f in range(2)],
        force_tracking_error=[div(ac("FT", f), env_steps) for f in range(2)],
        torque_mean=div(ac("TAU"), 12 * env_steps),
        torque_diff_max_mean=div(ac("DTM"), eps),
        pushes=ct("PUSHES"), push_falls=ct("PUSH_FALLS"),
        perturb_start_latched=gate_at > 0, perturb_start_at_record=gate_at - 1 if gate_at else None)
    return s


class EpisodeStats(EpisodeWindow):
    """The statistics of one DyrosDynamicWalk env (see the module docstring).  Buffers are allocated here, once."""

    CAUSES = CAUSES

    def __init__(self, env, spec=True):
        super().__init__(env, declare, K, "DWS_")
        self.body_names = list(env.model.body_names)          # (Gym rows: 8 and 16 are L_Foot_Link / R_Foot_Link)
        self.restart()

    def _bufs(self):
        N, f = self.num_envs, torch.float32
        return (self._in("root_states", f, shape=(N, 13)), self._in("contact_forces", f, shape=(N, self.env.num_bodies, 3)),
                self._in("env_state", f, numel=N * self.env._buf["env_state"].shape[1]))

    def record(self):
        """After a step, on the step's stream (DyrosDynamicWalk.step calls it)."""
        N = self.num_envs
        root, cf, es = self._bufs()
        self._launch("record", (N, root, cf, es, self._in("reset_buf", torch.int64, shape=(N,)), self._in("total_mass", torch.float32, numel=N),
                                self.st.data_ptr(), self.ac.data_ptr(), self.ct.data_ptr(), self.cause.data_ptr(),
                                float(self.env.max_episode_length), float(self.env.dt_policy)))

    def restart(self, env_ids: torch.Tensor = None):
        """Discards the running episode of env_ids (None: every env); their counters restart from progress_buf."""
        N = self.num_envs
        root, _cf, es = self._bufs()
        ids, n = None, N
        if env_ids is not None:
            ids = _req("env_ids", env_ids, torch.int32)
            n = ids.numel()
            if n == 0:
                return
        self._launch("restart", (N, ids.data_ptr() if ids is not None else None, n, root, es, self._in("progress_buf", torch.int64, shape=(N,)),
                                 self.st.data_ptr()))

    def summary(self) -> dict:
        return fold(self.raw(), self.num_envs, float(self.env.max_episode_length), self.body_names)


def format_line(s: dict) -> str:
    """One log line: cause fractions, the three most frequent contact bodies, mean length, push falls."""
    fr = "  ".join("%s %.3f" % (n, v) for n, v in s["cause_fractions"].items())
    top = sorted(s["contact_bodies"].items(), key=lambda kv: -kv[1])[:3]
    return "episodes %d: %s | contact bodies %s | mean length %.1f | push falls %d of %d pushes" % (
        s["episodes"], fr, ", ".join("%s %d" % kv for kv in top) or "-", s["mean_length"], s["push_falls"], s["pushes"])


def format_table(s: dict) -> str:
    """The whole summary as a plain-text table (examples/ppo_player.py --report)."""
    L = ["episode statistics: %d episodes over %d records" % (s["episodes"], s["records"]),
         "  termination causes (orientation together with a contact counts as contact):"]
    for n, v in s["causes"].items():
        L.append("    %-18s %8d  %.3f" % (n, v, s["cause_fractions"][n]))
    L.append("  bodies over 1 N at a non_foot_contact end (ground contact and self-collision together):")
    for n, v in sorted(s["contact_bodies"].items(), key=lambda kv: -kv[1]):
        L.append("    %-18s %8d" % (n, v))
    L.append("  episode length: mean %.1f  max %d  histogram %s" % (s["mean_length"], s["max_length"], s["length_hist"]))
    L.append("  mean return of finished episodes: %.4g" % s["mean_return"])
    L.append("  command tracking by commanded target_vel[0]:")
    L.append("    %-11s %8s %10s %10s %10s" % ("bin [m/s]", "episodes", "|v err|", "|dy| [m]", "dx/(v T)"))
    for b in s["command_bins"]:
        L.append("    %4.1f - %-4.1f %8d %10.4f %10.4f %10.4f" % (b["lo"], b["hi"], b["episodes"], b["vel_error"], b["lateral_drift"], b["distance_ratio"]))
    L.append("  sole loads: mean peak F_z L %.1f N  R %.1f N; peak > 1400 N: L %.3f  R %.3f; |force tracking| L %.2f  R %.2f" % (
        s["sole_peak_mean"][0], s["sole_peak_mean"][1], s["sole_over_1400"][0], s["sole_over_1400"][1],
        s["force_tracking_error"][0], s["force_tracking_error"][1]))
    L.append("  torques: mean |tau| %.3f  mean per-episode max |tau_t - tau_t-1| %.3f" % (s["torque_mean"], s["torque_diff_max_mean"]))
    L.append("  pushes: %d started, %d episodes ended during or within 250 steps of one (not by time limit)" % (s["pushes"], s["push_falls"]))
    L.append("  perturbation gate: %s" % ("latched at record %d" % s["perturb_start_at_record"] if s["perturb_start_latched"] else "not latched"))
    return "\n".join(L)
