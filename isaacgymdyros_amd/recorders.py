"""What the per-step recorders share on the host (DESIGN.md sections 16-20, 16a): Recorder, the base of EpisodeStats, AmpEpisodeStats,
RunTrace and GaitProfile; EpisodeWindow, what the two statistics classes have in common; and WALK, the table of DyrosDynamicWalk's
recorders, by which the env and config.validate_cfg validate, attach, record and restart them.

A recorder is a module of this package with K, EXPORTS and declare, and a class over one env object's bound buffers with record().  (The
learners' GameMeter is no Recorder: it is bound to no env and has a torch backend.)
"""
from __future__ import annotations

import importlib

from . import cbind

# (name: module, env attribute and cfg key sim.mi355.<name>; class; the method that discards what the recorder holds of envs after an
# explicit reset, or None), in the order of a step's launches
WALK = (
    ("episode_stats", "EpisodeStats", "restart"),          # termination causes and per-episode statistics (bool only)
    ("run_trace", "RunTrace", "arm"),                      # a ring of the last steps of chosen envs, optionally frozen at a fall
    ("gait_profile", "GaitProfile", None),                 # sole forces, contacts and joint tracking binned by mocap phase
)


def _module(name):
    return importlib.import_module("." + name, __package__)


def is_on(spec) -> bool:
    """Whether a cfg value switches a recorder on: anything but None and False ({} and True are the default spec)."""
    return spec is not None and spec is not False


def validate_all(cfg: dict, num_envs: int) -> None:
    """Every walk recorder's validate() of cfg sim.mi355.<name>: ValueError before anything is loaded or allocated."""
    mi = cfg["sim"].get("mi355", {})
    for name, _, _ in WALK:
        if name in mi:
            _module(name).validate(mi[name], num_envs)


def attach(env, mi355: dict) -> None:
    """env.<name> of every walk recorder: its object where mi355[<name>] switches it on, None otherwise (step() then makes no launch for it)."""
    for name, cls, _ in WALK:
        setattr(env, name, getattr(_module(name), cls)(env, mi355[name]) if is_on(mi355.get(name)) else None)
    if env.episode_stats is not None:
        env.extras["termination_cause"] = env.episode_stats.cause          # (record() fills it in place)


def record_all(env) -> None:
    """record() of every attached recorder, after a step and on its stream."""
    for name, _, _ in WALK:
        if getattr(env, name) is not None:
            getattr(env, name).record()


def restart_all(env, ids=None) -> None:
    """After an explicit reset of envs ids (None: every env): their running episodes are discarded, not counted, and their trace slots armed."""
    for name, _, hook in WALK:
        if hook is not None and getattr(env, name) is not None:
            getattr(getattr(env, name), hook)(ids)


class Recorder(cbind.Launcher):
    """The base of the recorders' classes: the entry points, the env and its device, the launch, and the env's buffers as checked pointers."""

    def __init__(self, env, declare):
        from . import _lib
        self.api = declare(_lib.load()[0])
        self.env, self.num_envs, self._tdev = env, env.num_envs, env._tdev

    def _in(self, name, dtype, **kw) -> int:
        """The pointer of env._buf[name], its dtype and shape or size checked.  For argument tuples built once: the env's buffers are bound
        once (load_state_dict copies into them), so no argument changes from call to call and a step pays one ctypes call."""
        from .ppo_update import _req
        return _req(name, self.env._buf[name], dtype, **kw).data_ptr()


def div(a, b):
    return a / b if b else float("nan")


class Window:
    """A summarize's doubles by name: ct("EPISODES"), ac("PK", 1) of the ABI with constants k and prefix p ("DWS_")."""

    def __init__(self, out, k, p):
        self.out, self.k, self.p = out, k, p

    def ct(self, name, i=0) -> int:
        return int(self.out[self.k[self.p + "CT_" + name] + i])

    def ac(self, name, i=0) -> float:
        return float(self.out[self.k[self.p + "CT_WORDS"] + self.k[self.p + "AC_" + name] + i])          # (SUM_AC = CT_WORDS)

    def head(self, causes: dict, body_names, max_episode_length: float) -> dict:
        """What both statistics summaries begin with; causes: name -> count."""
        eps, nl = self.ct("EPISODES"), self.k[self.p + "LEN_BINS"]
        bodies = {body_names[g]: self.ct("BODY", g) for g in range(len(body_names))}
        return dict(
            records=self.ct("RECORDS"), episodes=eps, causes=causes, cause_fractions={n: div(v, eps) for n, v in causes.items()},
            contact_bodies={n: v for n, v in bodies.items() if v},
            mean_length=div(self.ct("LEN_SUM"), eps), max_length=self.ct("LEN_MAX"),
            length_hist=[self.ct("LEN_HIST", i) for i in range(nl)], length_edges=[max_episode_length * i / nl for i in range(nl + 1)],
            mean_return=div(self.ac("RET"), eps), sole_peak_mean=[div(self.ac("PK", f), eps) for f in range(2)],
            record_calls=self.ct("CALLS"))


class EpisodeWindow(Recorder):
    """The base of EpisodeStats and AmpEpisodeStats: the per-env state st, the window's sums ac and counts ct, the published cause and the
    summarize output, sized from the module's constants k by prefix p; a window is read with raw() and restarted with reset_totals()."""

    def __init__(self, env, declare, k, p):
        import torch
        super().__init__(env, declare)
        self._window = k[p + "CT_WINDOW"]
        N, dev = self.num_envs, self._tdev
        self.st = torch.zeros(k[p + "ST_WORDS"], N, dtype=torch.int32, device=dev)
        self.ac = torch.zeros(k[p + "AC_WORDS"], N, dtype=torch.float32, device=dev)
        self.ct = torch.zeros(k[p + "CT_WORDS"], dtype=torch.int64, device=dev)          # (uint64 on the device side)
        self.cause = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.out = torch.zeros(k[p + "CT_WORDS"] + k[p + "AC_WORDS"], dtype=torch.float64, device=dev)

    def reset_totals(self):
        """Starts a new window."""
        self.ac.zero_()
        self.ct[:self._window].zero_()

    def raw(self) -> list:
        """The summarize's doubles (one launch, one device-to-host copy)."""
        self._launch("summarize", (self.num_envs, self.ac.data_ptr(), self.ct.data_ptr(), self.out.data_ptr()))
        return self.out.cpu().tolist()
