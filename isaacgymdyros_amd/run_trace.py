"""DyrosDynamicWalk's on-GPU run trace (include/dyros_trace.h, csrc/dw_trace.hip): a flight recorder.

Opt-in: cfg["sim"]["mi355"]["run_trace"] = {"env_ids": [..] | K, "depth": T, "hold": "never" | "fall" | "reset"} gives the env a
`run_trace` attribute (None otherwise).  K chosen envs (an int K: envs 0 .. K-1) each keep a ring of their last T steps.  Every step() then
makes one more launch, dwt_record, on the step's stream: one row per traced env with its root state, joint angles and velocities, what the
policy saw, the mocap target, actions, torques, sole forces, the largest other contact, the rewards and the reset flags (CHANNELS).  No
host sync and no allocation per step, so the launch sits inside a captured rollout graph like the step itself.

With hold "fall" a slot freezes at the step that ends its episode other than by the time limit ("reset": at any reset): its ring then holds
the approach to the fall, ending with the terminating step, until arm() releases it.

    record()            after a step (DyrosDynamicWalk.step calls it)
    held()              device bool [K], no sync
    arm(env_ids=None)   releases and clears the slots of env_ids (None: all); their episode count restarts from progress_buf
    retarget(env_ids)   traces K other envs from now on
    read(env_ids=None)  the rings as numpy arrays, oldest row first: one gather launch and one device-to-host copy
    drain(max_slots)    up to max_slots held slots read and armed again, with one device-to-host copy in all
    episodes(env_id)    an env's rows split at the reset flags
    save_npz(path, env_id), export_txt(dir, env_id)
    CHANNELS            name -> (offset, shape, kind) of a row's words

Explicit reset_idx(), load_state_dict() and construction arm the slots of the envs they touch.

Terminal rows: the step kernel resets an env in the launch that ends its episode, so in a row whose reset flag is set root_states, dof_pos,
dof_vel, target_vel and pert_on already belong to the new episode; contact forces, action_torque and the rewards are the ended episode's.
A fall is read from the rows before the flagged one, plus the flagged row's forces.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import cbind
from .ppo_update import _req
from .recorders import Recorder

K = cbind.constants("dyros_trace.h", "dwt_")
EXPORTS = list(cbind.signatures("dyros_trace.h", "dwt_"))
HOLD = {"never": K["DWT_HOLD_NEVER"], "fall": K["DWT_HOLD_FALL"], "reset": K["DWT_HOLD_RESET"]}
ROW_WORDS = K["DWT_ROW_WORDS"]
ROW_BYTES = 4 * ROW_WORDS
MAX_RING_BYTES = 1 << 30
FLAGS = {"reset": K["DWT_FLAG_RESET"], "time_limit": K["DWT_FLAG_TIME_LIMIT"], "pert_on": K["DWT_FLAG_PERT_ON"],
         "perturb_start": K["DWT_FLAG_PERT_START"], "timeout": K["DWT_FLAG_TIMEOUT"]}


def _ch(name, shape=None, kind="f"):
    n = K["DWT_LEN_" + name]
    return (K["DWT_CH_" + name], (n,) if shape is None else shape, kind)


# name -> (offset in 32-bit words, shape, 'f' float32 | 'i' int32); the spans tile the row in this order
CHANNELS = {
    "seen": _ch("SEEN", (), "i"), "epi_step": _ch("EPI_STEP", (), "i"), "flags": _ch("FLAGS", (), "i"), "nan_resets": _ch("NAN_RESETS", (), "i"),
    "root_states": _ch("ROOT"), "dof_pos": _ch("DOF_POS"), "dof_vel": _ch("DOF_VEL"), "qpos_noise": _ch("QPOS_NOISE"),
    "target_data_qpos": _ch("TARGET_QPOS"), "actions": _ch("ACTIONS"), "action_torque": _ch("TORQUE"), "foot_forces": _ch("FOOT_FORCE", (2, 3)),
    "non_foot_max": _ch("NF_MAX", ()), "non_foot_body": _ch("NF_BODY", ()), "target_data_force": _ch("TARGET_FORCE"),
    "target_vel": _ch("TARGET_VEL"), "magnitude": _ch("MAGNITUDE", ()), "phase": _ch("PHASE", ()), "time": _ch("TIME", ()),
    "rew_buf": _ch("REW", ()), "stacked_rewards": _ch("STACKED"), "pad": _ch("PAD"),
}


def declare(lib) -> dict:
    return cbind.declare(lib, "dyros_trace.h", "dwt_")


def resolve_env_ids(spec, num_envs: int) -> list:
    """The env id list of a cfg's run_trace["env_ids"]; ValueError for ids out of range or repeated."""
    if isinstance(spec, bool) or not isinstance(spec, (int, list, tuple)):
        raise ValueError("sim.mi355.run_trace.env_ids must be an int K (envs 0 .. K-1) or a list of env ids")
    ids = list(range(spec)) if isinstance(spec, int) else list(spec)
    if not ids:
        raise ValueError("sim.mi355.run_trace.env_ids names no env")
    if any(isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= i < num_envs for i in ids):
        raise ValueError("sim.mi355.run_trace.env_ids must be env ids in [0, %d)" % num_envs)
    if len(set(ids)) != len(ids):
        raise ValueError("sim.mi355.run_trace.env_ids repeats an env")
    return [int(i) for i in ids]


def validate(spec, num_envs: int) -> None:
    """Range checks of cfg sim.mi355.run_trace (config.validate_cfg); None or False: the trace is off."""
    if spec is None or spec is False:
        return
    if not isinstance(spec, dict):
        raise ValueError("sim.mi355.run_trace must be a dict with env_ids, depth and hold")
    unknown = set(spec) - {"env_ids", "depth", "hold"}
    if unknown:
        raise ValueError("sim.mi355.run_trace: unknown keys %s" % sorted(unknown))
    ids = resolve_env_ids(spec.get("env_ids", 64), num_envs)
    depth = spec.get("depth", 512)
    if isinstance(depth, bool) or not isinstance(depth, int) or depth < 1:
        raise ValueError("sim.mi355.run_trace.depth must be a positive integer, got %r" % (depth,))
    if spec.get("hold", "fall") not in HOLD:
        raise ValueError("sim.mi355.run_trace.hold must be one of %s, got %r" % (sorted(HOLD), spec.get("hold")))
    if len(ids) * depth * ROW_BYTES > MAX_RING_BYTES:
        raise ValueError("sim.mi355.run_trace: %d envs x %d steps x %d bytes is over 1 GiB" % (len(ids), depth, ROW_BYTES))


def decode(rows: np.ndarray) -> dict:
    """[..., DWT_ROW_WORDS] uint32 rows -> one array per channel, and `flags` as named bool arrays."""
    out = {}
    for name, (off, shape, kind) in CHANNELS.items():
        n = int(np.prod(shape, dtype=np.int64))
        v = rows[..., off:off + n].view(np.int32 if kind == "i" else np.float32)
        out[name] = v.reshape(rows.shape[:-1] + tuple(shape))
    out["flags"] = {name: (out["flags"] & bit) != 0 for name, bit in FLAGS.items()} | {"bits": out["flags"]}
    return out


def cut(r: dict, i: int) -> dict:
    """Entry i of a read() result, cut to its used rows: every channel [rows, ...], `flags` as named bool arrays, and the slot's scalars."""
    n = int(r["rows"][i])
    out = {k: v[i, :n] for k, v in r.items() if k in CHANNELS and k != "flags"}
    out["flags"] = {k: v[i, :n] for k, v in r["flags"].items()}
    out.update(env_id=int(r["env_ids"][i]), held=bool(r["held"][i]), cursor=int(r["cursor"][i]), falls=int(r["falls"][i]))
    return out


def split_episodes(one: dict) -> list:
    """The rows of a cut() split after every row whose reset flag is set: a list of dicts of arrays, oldest first.  The first piece may lack
    its start (the ring wrapped) and the last its end (the episode is running)."""
    n = len(one["seen"])
    if n == 0:
        return []
    ends = [int(i) + 1 for i in np.nonzero(one["flags"]["reset"])[0]]
    cuts = [0] + ends + ([n] if not ends or ends[-1] != n else [])
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        d = {k: v[a:b] for k, v in one.items() if isinstance(v, np.ndarray)}
        d["flags"] = {k: v[a:b] for k, v in one["flags"].items()}
        out.append(d)
    return out


def flat(one: dict) -> dict:
    """A cut() as save_npz writes it: one array per channel (no pad), `flags` as the raw bits and `flag_<name>` decoded."""
    d = {k: v for k, v in one.items() if k != "flags" and k != "pad"}
    d.update({"flag_" + k: v for k, v in one["flags"].items() if k != "bits"})
    d["flags"] = one["flags"]["bits"]
    return d


def write_npz(path: str, one: dict):
    np.savez(path, **flat(one))


def write_txt(directory: str, one: dict) -> list:
    """One tab-separated text file per channel, <channel>_env<id>.txt, one line per step (the separators of the reference's commented-out
    loggers, tasks/dyros_dynamic_walk.py:566-579).  Returns the paths."""
    os.makedirs(directory, exist_ok=True)
    paths = []
    for name, v in flat(one).items():
        if not isinstance(v, np.ndarray):
            continue
        paths.append(os.path.join(directory, "%s_env%d.txt" % (name, one["env_id"])))
        with open(paths[-1], "w") as f:
            for row in v.reshape(len(v), -1):
                f.write("\t".join(str(x) for x in (row.astype(int) if row.dtype == bool else row).tolist()) + "\n")
    return paths


class RunTrace(Recorder):
    """The trace of one DyrosDynamicWalk env (see the module docstring).  Buffers are allocated here, once."""

    CHANNELS = CHANNELS

    def __init__(self, env, spec: dict):
        super().__init__(env, declare)
        N, dev = self.num_envs, self._tdev
        validate(spec, N)
        self.depth = int(spec.get("depth", 512))
        self.hold = spec.get("hold", "fall")
        ids = resolve_env_ids(spec.get("env_ids", 64), N)
        self.num_slots = len(ids)
        self.ring = torch.zeros(self.num_slots, self.depth, ROW_WORDS, dtype=torch.int32, device=dev)
        self.ss = torch.zeros(K["DWT_SS_WORDS"], self.num_slots, dtype=torch.int32, device=dev)
        self.slot_env = torch.zeros(self.num_slots, dtype=torch.int32, device=dev)
        self.env_slot = torch.zeros(N, dtype=torch.int32, device=dev)
        p, f, i64 = self._in, torch.float32, torch.int64
        self._record_args = (
            N, self.num_slots, self.depth, HOLD[self.hold], self.slot_env.data_ptr(), p("root_states", f, shape=(N, 13)),
            p("dof_state", f, numel=N * 66), p("contact_forces", f, shape=(N, env.num_bodies, 3)),
            p("env_state", f, numel=N * env._buf["env_state"].shape[1]), p("rew_buf", f, numel=N), p("stacked_rewards", f, shape=(N, 15)),
            p("reset_buf", i64, shape=(N,)), p("timeout_buf", i64, shape=(N,)), float(env.max_episode_length), self.ss.data_ptr(),
            self.ring.data_ptr())
        self.retarget(ids)

    def retarget(self, env_ids):
        """Traces these envs (as many as before) from now on: every slot is cleared and armed."""
        ids = resolve_env_ids([int(i) for i in (env_ids.tolist() if hasattr(env_ids, "tolist") else env_ids)], self.num_envs)
        if len(ids) != self.num_slots:
            raise ValueError("retarget takes %d env ids (the rings are allocated once), got %d" % (self.num_slots, len(ids)))
        self.env_ids = ids
        self._slot_of = {e: s for s, e in enumerate(ids)}
        t = torch.tensor(ids, dtype=torch.int32, device=self.slot_env.device)
        self.slot_env.copy_(t)
        self.env_slot.fill_(-1)
        self.env_slot[t.long()] = torch.arange(self.num_slots, dtype=torch.int32, device=t.device)
        self.arm()

    def record(self):
        """After a step, on the step's stream (DyrosDynamicWalk.step calls it)."""
        self._launch("record", self._record_args)

    def arm(self, env_ids: torch.Tensor = None):
        """Releases and clears the slots of env_ids (None: every slot); envs that are not traced, or out of range, are ignored."""
        N = self.num_envs
        ids, n = None, N
        if env_ids is not None:
            ids = _req("env_ids", torch.as_tensor(env_ids, device=self.ss.device).to(torch.int32), torch.int32)
            n = ids.numel()
            if n == 0:
                return
        self._launch("arm", (N, self.num_slots, ids.data_ptr() if ids is not None else None, n, self._in("progress_buf", torch.int64, shape=(N,)),
                             self.env_slot.data_ptr(), self.ss.data_ptr()))

    def held(self) -> torch.Tensor:
        """Device bool [K], in slot order (self.env_ids); no sync."""
        return self.ss[K["DWT_SS_HELD"]] != 0

    def _gather(self, ids: torch.Tensor):
        """The rings, row counts and state words of the slots `ids` (device int32 [n]) and ids itself, with one device-to-host copy."""
        n = ids.numel()
        out = torch.empty(n, self.depth, ROW_WORDS, dtype=torch.int32, device=self.ss.device)
        rows = torch.empty(n, dtype=torch.int32, device=self.ss.device)
        self._launch("gather", (self.num_slots, self.depth, ids.data_ptr(), n, self.ss.data_ptr(), self.ring.data_ptr(), out.data_ptr(),
                                rows.data_ptr()))
        st = self.ss[:, ids.long()].t().contiguous()
        flat_ = torch.cat([out.reshape(-1), rows, st.reshape(-1), ids]).cpu().numpy()
        w = n * self.depth * ROW_WORDS
        return (flat_[:w].view(np.uint32).reshape(n, self.depth, ROW_WORDS), flat_[w:w + n].copy(),
                flat_[w + n:w + n + n * K["DWT_SS_WORDS"]].view(np.uint32).reshape(n, K["DWT_SS_WORDS"]), flat_[w + n + n * K["DWT_SS_WORDS"]:].copy())

    def _read(self, ids: torch.Tensor) -> dict:
        raw, rows, st, slots = self._gather(ids)
        out = decode(raw)
        out.update(rows=rows.astype(np.int64), env_ids=np.asarray([self.env_ids[s] for s in slots], np.int64), held=st[:, K["DWT_SS_HELD"]] != 0,
                   cursor=st[:, K["DWT_SS_CURSOR"]].astype(np.int64), falls=st[:, K["DWT_SS_FALLS"]].astype(np.int64))
        return out

    def read(self, env_ids=None) -> dict:
        """The rings of env_ids (None: every traced env, in slot order) as numpy arrays [n, depth, ...], oldest row first; `rows` [n] says
        how many are used (the others are zero).  Also `env_ids`, `flags` (named bool arrays), and the slots' `held`, `cursor`, `falls`.
        One gather launch and one device-to-host copy."""
        envs = list(self.env_ids) if env_ids is None else [int(e) for e in (env_ids.tolist() if hasattr(env_ids, "tolist") else env_ids)]
        for e in envs:
            if e not in self._slot_of:
                raise ValueError("env %d is not traced" % e)
        return self._read(torch.tensor([self._slot_of[e] for e in envs], dtype=torch.int32, device=self.ss.device))

    def drain(self, max_slots: int = None) -> list:
        """Up to max_slots held slots (None: all) as cut() dicts, and those slots armed again.  The slots are chosen and armed on the
        device: one gather launch, one arm launch and ONE device-to-host copy, whatever is held."""
        k = self.num_slots if max_slots is None else min(int(max_slots), self.num_slots)
        score, idx = torch.topk(self.held().to(torch.int32), k)          # (held slots first)
        r = self._read(idx.to(torch.int32))
        self.arm(torch.where(score > 0, self.slot_env[idx], -1))          # (-1: ignored; enqueued after the gather)
        return [cut(r, i) for i in range(k) if r["held"][i]]

    def one(self, env_id: int) -> dict:
        """read() of one env, cut to its used rows (cut())."""
        return cut(self.read([env_id]), 0)

    def episodes(self, env_id: int) -> list:
        """The used rows of one env split at the reset flags (split_episodes())."""
        return split_episodes(self.one(env_id))

    def save_npz(self, path: str, env_id: int):
        """One env's used rows as an .npz: one array per channel, `flags` as the raw bits and `flag_<name>` decoded."""
        write_npz(path, self.one(env_id))

    def export_txt(self, directory: str, env_id: int) -> list:
        """One tab-separated text file per channel and one line per step (write_txt())."""
        return write_txt(directory, self.one(env_id))
