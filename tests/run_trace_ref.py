"""A numpy restatement of the run trace (include/dyros_trace.h), written from the header's rules with array operations over
slots.  Used by tests/test_run_trace.py (against the g++ build of csrc/dw_trace.h) and tests/test_run_trace_gpu.py (against the HIP
kernels).  `Synth` is the synthetic input sequence both tests drive their side with."""
import numpy as np

from isaacgymdyros_amd import abi
from isaacgymdyros_amd.run_trace import CHANNELS, HOLD, K

E = abi.K
NB, ESW, W = E["DW_NUM_BODIES"], E["DW_ES_WORDS"], K["DWT_ROW_WORDS"]
LFOOT, RFOOT = 8, 16


def _put(rows, name, values):
    off, shape, kind = CHANNELS[name]
    n = int(np.prod(shape, dtype=np.int64))
    v = np.ascontiguousarray(values).reshape(len(rows), n)
    rows[:, off:off + n] = v.astype(np.int32).view(np.uint32) if kind == "i" else v.astype(np.float32).view(np.uint32)


def non_foot_max(cf):
    """cf [n, NB, 3] -> (|F| of the body with the largest norm among all bodies but the soles, its Gym row); the lowest row among equals.
    The norm is the step kernel's: ((x*x + y*y) + z*z) rounded after every operation, then the square root."""
    cf = cf.astype(np.float32)
    b = (cf[..., 0] * cf[..., 0]).astype(np.float32)
    b = (cf[..., 1].astype(np.float64) * cf[..., 1].astype(np.float64) + b.astype(np.float64)).astype(np.float32)          # fmaf: one rounding
    b = (cf[..., 2].astype(np.float64) * cf[..., 2].astype(np.float64) + b.astype(np.float64)).astype(np.float32)
    v = np.sqrt(b).astype(np.float32)
    key = (v.view(np.uint32) & np.uint32(0x7fffffff)).astype(np.int64)
    key[:, [LFOOT, RFOOT]] = -1
    g = np.argmax(key, axis=1)                                   # (the first of equal maxima)
    return v[np.arange(len(v)), g], g


class TraceRef:
    def __init__(self, num_envs, env_ids, depth, hold, max_len):
        self.n, self.k, self.depth, self.hold, self.ml = num_envs, len(env_ids), depth, HOLD[hold], np.float32(max_len)
        self.slot_env = np.asarray(env_ids, np.int32)
        self.env_slot = np.full(num_envs, -1, np.int32)
        self.env_slot[self.slot_env] = np.arange(self.k, dtype=np.int32)
        self.ring = np.zeros((self.k, depth, W), np.uint32)
        self.ss = np.zeros((K["DWT_SS_WORDS"], self.k), np.uint32)

    def arm(self, progress, ids=None):
        ids = np.arange(self.n) if ids is None else np.asarray(ids)
        ids = ids[(ids >= 0) & (ids < self.n)]
        ids = ids[self.env_slot[ids] >= 0]
        s = self.env_slot[ids]
        for w in ("CURSOR", "HELD", "SEEN", "FALLS"):
            self.ss[K["DWT_SS_" + w], s] = 0
        self.ss[K["DWT_SS_N"], s] = progress[ids].astype(np.uint32)

    def record(self, root, dof, cf, es, rew, stacked, reset, timeout):
        e = self.slot_env
        cur, held, n, seen, falls = (self.ss[K["DWT_SS_" + w]] for w in ("CURSOR", "HELD", "N", "SEEN", "FALLS"))
        seen += 1                                                # (views: the words change in place)
        live = held == 0
        esi = es.view(np.int32)
        n1 = n + 1
        rs = reset[e] != 0
        limit = n1.astype(np.float32) >= self.ml - np.float32(1.0)
        flags = (rs * K["DWT_FLAG_RESET"] + limit * K["DWT_FLAG_TIME_LIMIT"] + (esi[e, E["DW_ES_PERT_ON"]] != 0) * K["DWT_FLAG_PERT_ON"]
                 + (esi[e, E["DW_ES_PERT_START"]] != 0) * K["DWT_FLAG_PERT_START"] + (timeout[e] != 0) * K["DWT_FLAG_TIMEOUT"])
        rows = np.zeros((self.k, W), np.uint32)
        _put(rows, "seen", seen)
        _put(rows, "epi_step", n1)
        _put(rows, "flags", flags)
        _put(rows, "nan_resets", esi[e, E["DW_ES_NAN_RESETS"]])
        _put(rows, "root_states", root[e])
        _put(rows, "dof_pos", dof[e, :, 0])
        _put(rows, "dof_vel", dof[e, :, 1])
        for name, field in (("qpos_noise", "qpos_noise"), ("target_data_qpos", "target_data_qpos"), ("actions", "actions"),
                            ("action_torque", "action_torque"), ("target_data_force", "target_data_force"), ("target_vel", "target_vel"),
                            ("magnitude", "magnitude"), ("phase", "phase"), ("time", "time")):
            _put(rows, name, abi.es_view(es, field)[e])
        _put(rows, "foot_forces", cf[e][:, [LFOOT, RFOOT]])
        v, g = non_foot_max(cf[e])
        _put(rows, "non_foot_max", v)
        _put(rows, "non_foot_body", g.astype(np.float32))
        _put(rows, "rew_buf", rew[e])
        _put(rows, "stacked_rewards", stacked[e])
        s = np.nonzero(live)[0]
        self.ring[s, cur[s] % self.depth] = rows[s]
        cur[s] += 1
        fold = live & (cur >= K["DWT_CURSOR_FOLD"])
        cur[fold] = self.depth + cur[fold] % self.depth
        fall = live & rs & ~limit
        falls[fall] += 1
        n[live] = np.where(rs, 0, n1)[live]
        hold = live & rs if self.hold == HOLD["reset"] else fall if self.hold == HOLD["fall"] else np.zeros(self.k, bool)
        held[hold] = 1

    def gather(self, slots):
        out = np.zeros((len(slots), self.depth, W), np.uint32)
        nr = np.zeros(len(slots), np.int32)
        for i, s in enumerate(slots):
            if not 0 <= s < self.k:                              # (a slot id out of range: zero rows)
                continue
            c = int(self.ss[K["DWT_SS_CURSOR"], s])
            m = min(c, self.depth)
            nr[i] = m
            for r in range(m):
                out[i, r] = self.ring[s, (c - m + r) % self.depth]
        return out, nr


class Synth:
    """Random step buffers for n envs; reset_buf is scripted from each env's own step count so that falls (random), time limits (count
    reaching max_len - 1) and both occur."""

    def __init__(self, n, max_len, seed):
        self.rng = np.random.default_rng(seed)
        self.n, self.ml = n, max_len
        self.count = np.zeros(n, np.int64)                       # progress_buf of the scripted envs
        self.es = np.zeros((n, ESW), np.float32)
        self.esi = self.es.view(np.int32)

    def step(self, fall_p=0.15):
        r, n = self.rng, self.n
        f = lambda *s: r.normal(0, 1, s).astype(np.float32)          # noqa: E731
        self.root, self.dof = f(n, 13), f(n, 33, 2)
        self.cf = (f(n, NB, 3) * (r.random((n, NB, 1)) < 0.1) * 30).astype(np.float32)
        self.es[:] = f(n, ESW)
        self.esi[:, E["DW_ES_PERT_ON"]] = r.random(n) < 0.3
        self.esi[:, E["DW_ES_PERT_START"]] = r.random(n) < 0.5
        self.esi[:, E["DW_ES_NAN_RESETS"]] = r.integers(0, 5, n)
        self.rew, self.stacked = f(n), f(n, 15)
        self.count += 1
        limit = self.count.astype(np.float32) >= np.float32(self.ml) - 1
        self.reset = ((r.random(n) < fall_p) | limit).astype(np.int64)
        self.timeout = (limit & (r.random(n) < 0.8)).astype(np.int64)
        self.count[self.reset != 0] = 0
        return (self.root, self.dof, self.cf, self.es, self.rew, self.stacked, self.reset, self.timeout)
