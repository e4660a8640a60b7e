"""The learners' episode-return meter and best-reward checkpoint policy (include/dyros_meter.h, csrc/dw_meter.hip).

GameMeter restates what the reference learner keeps per step -- current_rewards, current_lengths and the two rl_games AverageMeter objects
game_rewards / game_lengths over the last `games_to_track` finished episodes (a2c_common_dyros.py:663-684, amp_continuous.py:126-143) -- as
one launch after env.step: no host sync, no allocation, no argument that changes between calls, so it sits inside a captured rollout step.
It is learner-side: it sees (reward, done) and optionally the stacked reward terms, so one implementation serves both tasks.

    record(rew, done, stacked=None)   after a step, on the current stream
    summary()                         one device-to-host copy: current_size, mean_reward (column 0), mean_rewards [cols], mean_length (the
                                      sliding window's), games / discarded / window_mean_reward / window_mean_length (since the last clear())
    clear()                           AverageMeter.clear() and the totals; the running episodes go on

A finished episode whose return is not finite is discarded and counted (`discarded`), not averaged: the one difference from the reference.
backend "torch" is the same rule in torch ops (it syncs with the host): for CPU runs and the tests.

BestCheckpoints is the reference's save policy around that mean (a2c_common_dyros.py:1039-1075), with no torch in it.
"""
from __future__ import annotations

import numpy as np

from . import cbind

K = cbind.constants("dyros_meter.h", "dwm_")
EXPORTS = list(cbind.signatures("dyros_meter.h", "dwm_"))
COLS_MAX = K["DWM_COLS_MAX"]
LAST_MEAN_REWARDS = -100500          # rl_games' start value of last_mean_rewards (a2c_common_dyros.py:582)


def declare(lib) -> dict:
    return cbind.declare(lib, "dyros_meter.h", "dwm_")


def _unpack(ms: np.ndarray, cols: int) -> dict:
    """The summary of an ms array (numpy uint32 [DWM_MS_WORDS])."""
    f = ms.view(np.float32)
    games = int(ms.view(np.uint64)[K["DWM_MS_GAMES"] // 2])
    d = ms.view(np.float64)
    means = [float(x) for x in f[K["DWM_MS_MEAN"]:K["DWM_MS_MEAN"] + cols]]
    return {"current_size": int(ms[K["DWM_MS_CURRENT_SIZE"]]), "mean_reward": means[0], "mean_rewards": means,
            "mean_length": float(f[K["DWM_MS_MEAN_LEN"]]), "games": games, "discarded": int(ms.view(np.uint64)[K["DWM_MS_DISCARDED"] // 2]),
            "window_mean_reward": float(d[K["DWM_MS_SUM_RET"] // 2]) / games if games else 0.0,
            "window_mean_length": float(d[K["DWM_MS_SUM_LEN"] // 2]) / games if games else 0.0}


def format_line(s: dict) -> str:
    """One log line of a summary()."""
    if s["current_size"] == 0:
        return "games: none finished yet"
    return ("games: mean return %.4f  mean length %.1f  over the last %d  (%d since the start of the run%s)"
            % (s["mean_reward"], s["mean_length"], s["current_size"], s["games"], ", %d discarded" % s["discarded"] if s["discarded"] else ""))


class GameMeter:
    """See the module docstring.  Buffers are allocated here, once."""

    def __init__(self, num_envs: int, device, cols: int = 1, games_to_track: int = 100, backend: str = "hip"):
        import torch
        if backend not in ("hip", "torch"):
            raise ValueError("GameMeter: backend must be 'hip' or 'torch', got %r" % (backend,))
        if isinstance(num_envs, bool) or not isinstance(num_envs, int) or num_envs < 1:
            raise ValueError("GameMeter: num_envs must be a positive integer, got %r" % (num_envs,))
        if isinstance(cols, bool) or not isinstance(cols, int) or not 1 <= cols <= COLS_MAX:
            raise ValueError("GameMeter: cols must be in [1, %d], got %r" % (COLS_MAX, cols))
        if isinstance(games_to_track, bool) or not isinstance(games_to_track, int) or not 1 <= games_to_track < 2 ** 31:
            raise ValueError("GameMeter: games_to_track must be a positive integer, got %r" % (games_to_track,))
        self.num_envs, self.cols, self.max_size, self.backend = num_envs, cols, games_to_track, backend
        self.device = torch.device(device)
        if backend == "hip":
            if self.device.type != "cuda":
                raise ValueError("GameMeter: backend 'hip' needs a GPU device, got %s (backend='torch' runs anywhere)" % self.device)
            from . import _lib
            self.api = declare(_lib.load()[0])
            words = self.api["work_words"](num_envs, cols)
            if words < 0:
                cbind.check(self.api, -1)
            self.cur = torch.zeros(cols + 1, num_envs, dtype=torch.float32, device=self.device)
            self.ms = torch.zeros(K["DWM_MS_WORDS"], dtype=torch.int32, device=self.device)
            self.work = torch.zeros(words, dtype=torch.int32, device=self.device)
        else:
            self.cur = torch.zeros(cols + 1, num_envs, dtype=torch.float32, device=self.device)
            self._reset_torch()

    # ------------------------------------------------------------------------------------------------ arguments
    def _arg(self, name, t, dtype, shape=None, numel=None):
        """ppo_update._req, with the device being this meter's."""
        import torch
        if not torch.is_tensor(t):
            raise ValueError("%s: a tensor is required, got %r" % (name, type(t).__name__))
        if t.dtype != dtype:
            raise ValueError("%s: dtype %s, expected %s" % (name, t.dtype, dtype))
        if t.device != self.device and not (t.device.type == self.device.type == "cuda" and self.device.index is None):
            raise ValueError("%s: must live on %s (it is on %s)" % (name, self.device, t.device))
        if not t.is_contiguous():
            raise ValueError("%s: must be contiguous (shape %r, strides %r)" % (name, tuple(t.shape), t.stride()))
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError("%s: shape %r, expected %r" % (name, tuple(t.shape), tuple(shape)))
        if numel is not None and t.numel() != numel:
            raise ValueError("%s: %d elements (shape %r), expected %d" % (name, t.numel(), tuple(t.shape), numel))
        return t

    def _done(self, done):
        import torch
        if torch.is_tensor(done) and done.dtype != torch.int64 and (done.dtype == torch.bool or done.dtype.is_floating_point):
            done = (done != 0).to(torch.int64)          # (a bool or float done: cast; inside a capture this is one more small launch)
        return self._arg("done", done, torch.int64, numel=self.num_envs)

    def record(self, rew, done, stacked=None):
        """After a step: rew [N] (or [N, 1]) float32, done [N] int64 (bool and float are cast), stacked [N, S >= cols - 1] float32 when
        cols > 1.  Tensors are checked like every kernel argument of this package: dtype, size, contiguity and device."""
        import torch
        N, C = self.num_envs, self.cols
        rew = self._arg("rew", rew, torch.float32, numel=N)
        done = self._done(done)
        if C > 1:
            if stacked is None:
                raise ValueError("stacked: cols = %d needs the stacked reward terms" % C)
            stacked = self._arg("stacked", stacked, torch.float32)
            if stacked.dim() != 2 or stacked.shape[0] != N or stacked.shape[1] < C - 1:
                raise ValueError("stacked: shape %r, expected (%d, >= %d)" % (tuple(stacked.shape), N, C - 1))
        if self.backend == "torch":
            return self._record_torch(rew.reshape(N), done, stacked)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        cbind.check(self.api, self.api["record"](N, C, self.max_size, rew.data_ptr(), stacked.data_ptr() if C > 1 else None,
                                                 stacked.shape[1] if C > 1 else 0, done.data_ptr(), self.cur.data_ptr(), self.ms.data_ptr(),
                                                 self.work.data_ptr(), stream))

    def clear(self):
        if self.backend == "torch":
            return self._reset_torch()
        import torch
        cbind.check(self.api, self.api["clear"](self.ms.data_ptr(), self.work.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream))

    def summary(self) -> dict:
        if self.backend == "torch":
            t = self._t
            games = t["games"]
            means = [float(x) for x in t["mean"][:self.cols]]
            return {"current_size": t["current_size"], "mean_reward": means[0], "mean_rewards": means, "mean_length": float(t["mean"][self.cols]),
                    "games": games, "discarded": t["discarded"], "window_mean_reward": t["sum_ret"] / games if games else 0.0,
                    "window_mean_length": t["sum_len"] / games if games else 0.0}
        return _unpack(self.ms.cpu().numpy().view(np.uint32), self.cols)

    # ------------------------------------------------------------------------------------------------ the rule in torch ops
    def _reset_torch(self):
        import torch
        self._t = {"current_size": 0, "mean": torch.zeros(self.cols + 1, dtype=torch.float32), "games": 0, "discarded": 0, "sum_ret": 0.0,
                   "sum_len": 0.0}

    def _record_torch(self, rew, done, stacked):
        import torch
        C, t = self.cols, self._t
        self.cur[0] += rew
        if C > 1:
            self.cur[1:C] += stacked[:, :C - 1].t()
        self.cur[C] += 1.0
        dn = done != 0
        in_d = dn & torch.isfinite(self.cur[:C]).all(dim=0)
        k = int(in_d.sum())
        if k > 0:
            x = self.cur[:, in_d]
            tot = x.double().sum(dim=1)                       # (the sums without rounding; the division and the window in float32)
            new_mean = (tot.float() / torch.tensor(float(k), dtype=torch.float32, device=tot.device)).cpu()
            size = min(k, self.max_size)
            old = min(self.max_size - size, t["current_size"])
            f = lambda v: torch.tensor(float(v), dtype=torch.float32)          # noqa: E731
            t["mean"] = (t["mean"] * f(old) + new_mean * f(size)) / f(old + size)
            t["current_size"] = old + size
            t["games"] += k
            t["sum_ret"] += float(tot[0])
            t["sum_len"] += float(tot[C])
        t["discarded"] += int(dn.sum()) - k
        self.cur[:, dn] = 0.0


def _rew(x) -> str:
    """str() of the mean as the reference prints it: a numpy float32 (AverageMeter.get_mean() is a float32 array)."""
    return str(np.float32(x))


class BestCheckpoints:
    """The reference learner's save policy (a2c_common_dyros.py:1039-1075) as names to write; the caller saves.  After every epoch in which
    the meter holds at least one game:
        last_<name>_ep_<n>_rew_<r>   when epoch % save_frequency == 0 (save_frequency > 0) and the mean is not above the best so far
        <name>                       when the mean is above the best so far and epoch >= save_best_after: it becomes the best
        <name>_ep_<n>_rew_<r>        also, when that new best is above score_to_win; should_exit is then set
    and final(epoch, mean_reward) names the file of the end of the run, last_<name>ep<n>rew<r>.  `last_mean_rewards` starts at rl_games'
    -100500 or at a checkpoint's value, so a resumed run keeps its best.  The best moves only where <name> is written: before
    save_best_after a mean above it writes nothing, as in the reference.  The reference prints <r> of the last file as the whole array
    of means ("[1.5]"); here it is the first mean, as in the other names."""

    def __init__(self, name: str, save_frequency: int, save_best_after: int, score_to_win: float, last_mean_rewards: float = LAST_MEAN_REWARDS):
        self.name, self.save_frequency, self.save_best_after = str(name), int(save_frequency), int(save_best_after)
        self.score_to_win, self.last_mean_rewards = float(score_to_win), last_mean_rewards

    def after_epoch(self, epoch: int, mean_reward: float):
        files, should_exit = [], False
        tag = "%s_ep_%d_rew_%s" % (self.name, epoch, _rew(mean_reward))
        if self.save_frequency > 0 and epoch % self.save_frequency == 0 and mean_reward <= self.last_mean_rewards:
            files.append("last_" + tag)
        if mean_reward > self.last_mean_rewards and epoch >= self.save_best_after:
            self.last_mean_rewards = mean_reward
            files.append(self.name)
            if self.last_mean_rewards > self.score_to_win:
                files.append(tag)
                should_exit = True
        return files, should_exit

    def final(self, epoch: int, mean_reward: float) -> str:
        return "last_%sep%drew%s" % (self.name, epoch, _rew(mean_reward))
