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

from . import _lib, cbind
from .cbind import check as _check
from .ppo_update import _req

K = cbind.constants("dyros_stats.h", "dws_")
K["DWS_SUM_AC"] = K["DWS_CT_WORDS"]                                  # (defined by expression in the header)
K["DWS_SUM_WORDS"] = K["DWS_CT_WORDS"] + K["DWS_AC_WORDS"]
EXPORTS = list(cbind.signatures("dyros_stats.h", "dws_"))
CAUSES = {0: "none", 1: "time_limit", 2: "non_foot_contact", 3: "orientation", 4: "non_finite"}
CMD_EDGES = (0.0, 0.2, 0.4, 0.6, 0.8)


def declare(lib) -> dict:
    return cbind.declare(lib, "dyros_stats.h", "dws_")


def fold(out, num_envs: int, max_episode_length: float, body_names) -> dict:
    """The summary dict from dws_summarize's [DWS_SUM_WORDS] doubles (a sequence of Python floats)."""
    k = K
    ct = lambda i: int(out[i])                                   # noqa: E731
    ac = lambda i: float(out[k["DWS_SUM_AC"] + i])               # noqa: E731
    eps = ct(k["DWS_CT_EPISODES"])
    records = ct(k["DWS_CT_RECORDS"])
    env_steps = records * num_envs
    div = lambda a, b: a / b if b else float("nan")              # noqa: E731
    causes = {CAUSES[c]: ct(k["DWS_CT_CAUSE"] + c) for c in range(1, 5)}
    bodies = {body_names[g]: ct(k["DWS_CT_BODY"] + g) for g in range(len(body_names))}
    bins = []
    for b in range(k["DWS_CMD_BINS"]):
        ne, nr, nq = ct(k["DWS_CT_BIN_EP"] + b), ct(k["DWS_CT_BIN_ROOT"] + b), ct(k["DWS_CT_BIN_RATIO"] + b)
        bins.append(dict(lo=CMD_EDGES[b], hi=CMD_EDGES[b + 1], episodes=ne, vel_error=div(ac(k["DWS_AC_VERR"] + b), nr),
                         lateral_drift=div(ac(k["DWS_AC_DRIFT"] + b), nr), distance_ratio=div(ac(k["DWS_AC_RATIO"] + b), nq),
                         ratio_episodes=nq))
    gate_at = ct(k["DWS_CT_GATE_AT"])
    return dict(
        records=records, episodes=eps, causes=causes,
        cause_fractions={n: div(v, eps) for n, v in causes.items()},
        contact_bodies={n: v for n, v in bodies.items() if v},
        mean_length=div(ct(k["DWS_CT_LEN_SUM"]), eps), max_length=ct(k["DWS_CT_LEN_MAX"]),
        length_hist=[ct(k["DWS_CT_LEN_HIST"] + i) for i in range(k["DWS_LEN_BINS"])],
        length_edges=[max_episode_length * i / k["DWS_LEN_BINS"] for i in range(k["DWS_LEN_BINS"] + 1)],
        mean_return=div(ac(k["DWS_AC_RET"]), eps),
        command_bins=bins,
        sole_peak_mean=[div(ac(k["DWS_AC_PK"] + f), eps) for f in range(2)],
        sole_over_1400=[div(ct(k["DWS_CT_PK_OVER"] + f), eps) for f in range(2)],
        force_tracking_error=[div(ac(k["DWS_AC_FT"] + f), env_steps) for f in range(2)],
        torque_mean=div(ac(k["DWS_AC_TAU"]), 12 * env_steps),
        torque_diff_max_mean=div(ac(k["DWS_AC_DTM"]), eps),
        pushes=ct(k["DWS_CT_PUSHES"]), push_falls=ct(k["DWS_CT_PUSH_FALLS"]),
        perturb_start_latched=gate_at > 0, perturb_start_at_record=gate_at - 1 if gate_at else None,
        record_calls=ct(k["DWS_CT_CALLS"]))


class EpisodeStats:
    """The statistics of one DyrosDynamicWalk env (see the module docstring).  Buffers are allocated here, once."""

    CAUSES = CAUSES

    def __init__(self, env):
        self.api = declare(_lib.load()[0])
        self.env = env
        N, dev = env.num_envs, env._tdev
        self.num_envs = N
        self.st = torch.zeros(K["DWS_ST_WORDS"], N, dtype=torch.int32, device=dev)
        self.ac = torch.zeros(K["DWS_AC_WORDS"], N, dtype=torch.float32, device=dev)
        self.ct = torch.zeros(K["DWS_CT_WORDS"], dtype=torch.int64, device=dev)          # (uint64 on the device side)
        self.cause = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.out = torch.zeros(K["DWS_SUM_WORDS"], dtype=torch.float64, device=dev)
        self.body_names = list(env.model.body_names)          # (Gym rows: 8 and 16 are L_Foot_Link / R_Foot_Link)
        self.restart()

    def _stream(self):
        return torch.cuda.current_stream(self.env._tdev).cuda_stream

    def _bufs(self):
        b, N = self.env._buf, self.num_envs
        return (_req("root_states", b["root_states"], torch.float32, shape=(N, 13)),
                _req("contact_forces", b["contact_forces"], torch.float32, shape=(N, self.env.num_bodies, 3)),
                _req("env_state", b["env_state"], torch.float32, numel=N * b["env_state"].shape[1]))

    def record(self):
        """After a step, on the step's stream (DyrosDynamicWalk.step calls it)."""
        b, N = self.env._buf, self.num_envs
        root, cf, es = self._bufs()
        rb = _req("reset_buf", b["reset_buf"], torch.int64, shape=(N,))
        tm = _req("total_mass", b["total_mass"], torch.float32, numel=N)
        _check(self.api, self.api["record"](N, root.data_ptr(), cf.data_ptr(), es.data_ptr(), rb.data_ptr(), tm.data_ptr(), self.st.data_ptr(),
                                            self.ac.data_ptr(), self.ct.data_ptr(), self.cause.data_ptr(), float(self.env.max_episode_length),
                                            float(self.env.dt_policy), self._stream()))

    def restart(self, env_ids: torch.Tensor = None):
        """Discards the running episode of env_ids (None: every env); their counters restart from progress_buf."""
        b, N = self.env._buf, self.num_envs
        root, _cf, es = self._bufs()
        pb = _req("progress_buf", b["progress_buf"], torch.int64, shape=(N,))
        ids, n = None, N
        if env_ids is not None:
            ids = _req("env_ids", env_ids, torch.int32)
            n = ids.numel()
            if n == 0:
                return
        _check(self.api, self.api["restart"](N, ids.data_ptr() if ids is not None else None, n, root.data_ptr(), es.data_ptr(), pb.data_ptr(),
                                             self.st.data_ptr(), self._stream()))

    def reset_totals(self):
        """Starts a new window."""
        self.ac.zero_()
        self.ct[:K["DWS_CT_WINDOW"]].zero_()

    def raw(self) -> list:
        """dws_summarize's doubles (one launch, one device-to-host copy)."""
        _check(self.api, self.api["summarize"](self.num_envs, self.ac.data_ptr(), self.ct.data_ptr(), self.out.data_ptr(), self._stream()))
        return self.out.cpu().tolist()

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
