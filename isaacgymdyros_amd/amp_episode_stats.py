"""TocabiAMPLower's on-GPU episode statistics (include/dyros_amp_stats.h, csrc/dw_amp_stats.hip).

Opt-in: cfg["sim"]["mi355"]["amp_episode_stats"] = True gives the env an `episode_stats` attribute (None otherwise).  Every step() then
makes one more launch, dwe_record, on the step's stream: why each env's step would end its episode (`extras["termination_cause"]`, a uint8
[N] bit mask overwritten in place: CAUSE_BITS), and per-episode and per-step sums folded into a window.  No host sync and no allocation per
step, so the launch sits inside a captured step like the step itself.  (`episode_stats` in a TocabiAMPLower cfg is NOT this feature: that
key belongs to DyrosDynamicWalk.)

    summary()        the window since construction or the last reset_totals(), as a dict: one reduction launch and one device-to-host copy
    reset_totals()   starts a new window (running episodes keep their counters)
    restart(ids)     forgets the running episode of the envs (a torch fill); construction calls it

TocabiAMPLower resets in reset_done(), after the step, so the record needs no hook in any reset path: an env whose progress_buf does not
continue its previous record's starts a new episode, and a running episode that is cut off that way counts as `discarded`.
"""
from __future__ import annotations

import torch

from . import cbind
from .ppo_update import _req
from .recorders import EpisodeWindow, Window, div
from .tocabi_amp_lower import REWARD_NAMES

K = cbind.constants("dyros_amp_stats.h", "dwe_")
K["DWE_SUM_AC"] = K["DWE_CT_WORDS"]                                  # (defined by expression in the header)
K["DWE_SUM_WORDS"] = K["DWE_CT_WORDS"] + K["DWE_AC_WORDS"]
EXPORTS = list(cbind.signatures("dyros_amp_stats.h", "dwe_"))
CAUSE_BITS = {"time_limit": K["DWE_C_TIME"], "non_foot_contact": K["DWE_C_CONTACT"], "root_low": K["DWE_C_LOW"], "foot_high": K["DWE_C_FLY"],
              "tilt": K["DWE_C_TILT"]}


def declare(lib) -> dict:
    return cbind.declare(lib, "dyros_amp_stats.h", "dwe_")


def mask_name(m: int) -> str:
    return "+".join(n for n, b in CAUSE_BITS.items() if m & b) or "none"


def fold(out, max_episode_length: float, body_names, command_x) -> dict:
    """The summary dict from dwe_summarize's [DWE_SUM_WORDS] doubles (a sequence of Python floats)."""
    w = Window(out, K, "DWE_")
    ct, ac = w.ct, w.ac
    masks = {m: ct("MASK", m) for m in range(K["DWE_MASKS"])}
    s = w.head({n: sum(v for m, v in masks.items() if m & b) for n, b in CAUSE_BITS.items()}, body_names, max_episode_length)
    samples = ct("SAMPLES")
    lo, hi = float(command_x[0]), float(command_x[1])
    nb = K["DWE_CMD_BINS"]
    bins = []
    for b in range(nb):
        steps = ac("VCNT", b)
        bins.append(dict(lo=lo + (hi - lo) * b / nb, hi=lo + (hi - lo) * (b + 1) / nb, steps=int(round(steps)),
                         x_vel_error=div(ac("VERR", b), steps)))
    s.update(
        discarded=ct("DISCARDED"), unreset_steps=ct("UNRESET"), nonfinite_steps=ct("NONFINITE"), sampled_steps=samples,
        cause_masks={mask_name(m): v for m, v in masks.items() if v},
        reward_terms={n: div(ac("REW", i), samples) for i, n in enumerate(REWARD_NAMES)},
        command_bins=bins,
        yaw_vel_error=div(ac("YAW"), samples),
        sole_over_threshold=[div(ct("SOLE_OVER", f), samples) for f in range(2)])
    return s


class AmpEpisodeStats(EpisodeWindow):
    """The statistics of one TocabiAMPLower env (see the module docstring).  Buffers are allocated here, once."""

    CAUSE_BITS = CAUSE_BITS

    def __init__(self, env):
        super().__init__(env, declare, K, "DWE_")
        N = self.num_envs
        self.body_names = list(env._phys.model.body_names)          # (Gym rows: 8 and 16 are L_Foot_Link / R_Foot_Link)
        assert len(self.body_names) == K["DWE_BODIES"]
        nb = env.num_bodies
        # the step's buffers: bound once (the env updates them in place and never re-binds them)
        self._args = (N, _req("root_states", env._root_states, torch.float32, shape=(N, 13)).data_ptr(),
                      _req("contact_forces", env._contact_forces, torch.float32, shape=(N, nb, 3)).data_ptr(),
                      _req("rigid_body_pos", env._rigid_body_pos, torch.float32, shape=(N, nb, 3)).data_ptr(),
                      _req("commands", env.commands, torch.float32, shape=(N, 3)).data_ptr(),
                      _req("rew_buf", env.rew_buf, torch.float32, shape=(N,)).data_ptr(),
                      _req("reward_values", env._reward_values, torch.float32, shape=(N, 9)).data_ptr(),
                      _req("reset_buf", env.reset_buf, torch.int64, shape=(N,)).data_ptr(),
                      _req("progress_buf", env.progress_buf, torch.int64, shape=(N,)).data_ptr(),
                      _req("total_mass", env.total_mass, torch.float32, numel=N).data_ptr(),
                      self.st.data_ptr(), self.ac.data_ptr(), self.ct.data_ptr(), self.cause.data_ptr(),
                      float(env.max_episode_length), float(env._termination_height), int(bool(env._enable_early_termination)),
                      float(env.c_x[0]), float(env.c_x[1]))
        self.restart()

    def record(self):
        """After a step, on the step's stream (the last call of TocabiAMPLower._step_body)."""
        self._launch("record", self._args)

    def restart(self, env_ids: torch.Tensor = None):
        """Forgets the running episode of env_ids (None: every env): it is not counted, and the env's next record starts a new one."""
        if env_ids is None:
            self.st[K["DWE_ST_N"]].fill_(-1)
        else:
            self.st[K["DWE_ST_N"]].index_fill_(0, env_ids.to(self.st.device).long(), -1)

    def summary(self) -> dict:
        return fold(self.raw(), float(self.env.max_episode_length), self.body_names, self.env.c_x)


def format_line(s: dict) -> str:
    """One log line: cause fractions, the three most frequent contact bodies, mean length and return."""
    fr = "  ".join("%s %.3f" % (n, v) for n, v in s["cause_fractions"].items())
    top = sorted(s["contact_bodies"].items(), key=lambda kv: -kv[1])[:3]
    return "episodes %d: %s | contact bodies %s | mean length %.1f | mean return %.3f | discarded %d" % (
        s["episodes"], fr, ", ".join("%s %d" % kv for kv in top) or "-", s["mean_length"], s["mean_return"], s["discarded"])


def format_table(s: dict) -> str:
    """The whole summary as a plain-text table (examples/amp_player.py --report)."""
    L = ["episode statistics: %d episodes over %d records (%d discarded, %d unreset steps, %d non-finite steps)" % (
        s["episodes"], s["records"], s["discarded"], s["unreset_steps"], s["nonfinite_steps"]),
         "  termination causes (an episode counts under every term that fired):"]
    for n, v in s["causes"].items():
        L.append("    %-18s %8d  %.3f" % (n, v, s["cause_fractions"][n]))
    L.append("  by combination:")
    for n, v in sorted(s["cause_masks"].items(), key=lambda kv: -kv[1]):
        L.append("    %-40s %8d" % (n, v))
    L.append("  bodies with a contact-force component over 1 at a non_foot_contact end:")
    for n, v in sorted(s["contact_bodies"].items(), key=lambda kv: -kv[1]):
        L.append("    %-18s %8d" % (n, v))
    L.append("  episode length: mean %.1f  max %d  histogram %s" % (s["mean_length"], s["max_length"], s["length_hist"]))
    L.append("  mean return of finished episodes: %.4g" % s["mean_return"])
    L.append("  mean reward terms per step:")
    for n, v in s["reward_terms"].items():
        L.append("    %-30s %10.5f" % (n, v))
    L.append("  command tracking by commands[0], per step:")
    L.append("    %-15s %10s %12s" % ("bin [m/s]", "steps", "|v_x err|"))
    for b in s["command_bins"]:
        L.append("    %6.3f - %-6.3f %10d %12.4f" % (b["lo"], b["hi"], b["steps"], b["x_vel_error"]))
    L.append("  mean |yaw rate error| per step: %.4f" % s["yaw_vel_error"])
    L.append("  sole loads: mean per-episode peak F_z / weight L %.2f  R %.2f; steps over 1.4 x weight: L %.4f  R %.4f" % (
        s["sole_peak_mean"][0], s["sole_peak_mean"][1], s["sole_over_threshold"][0], s["sole_over_threshold"][1]))
    return "\n".join(L)
