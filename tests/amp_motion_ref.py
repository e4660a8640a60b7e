"""TEST INFRASTRUCTURE ONLY -- what the device-resident motion library computes (isaacgymdyros_amd/csrc/dw_amp_motion.h), restated on the
host from TocabiLowerMotionLib.device_table(): the float64 index math in numpy, the float32 blends in torch on the CPU (the operations
get_motion_state performs), and the three generator words dw_amp_reset_done_motion draws a start from (on the Philox function of
oracle/amp_draws.py).  Also the small synthetic motion sets the tests of the device path share."""
import os

import numpy as np
import torch

from isaacgymdyros_amd import motion_lib as ML
from oracle import amp_draws
from tests import amp_motion_synth as SY

DS_MOTION = 15          # the generator stream of a resetting env's start (csrc/dw_amp_step.h)
Q, QV, RP, RR, RV, RA, KEY = slice(0, 12), slice(12, 24), slice(24, 27), slice(27, 31), slice(31, 34), slice(34, 37), slice(37, 43)


def write_small(dirname: str) -> str:
    """Three motions of unequal length cut from the synthetic tables (rows 0-499 hold the root rotation, 500-999 turn it by 1e-4 rad a
    frame, from 1000 on by up to 0.2 rad), one played backwards, unequal weights.  Returns the yaml's path."""
    for k, rows in enumerate((700, 1300, 1100)):
        np.savetxt(os.path.join(dirname, "small%d.txt" % k), SY.table(k)[:rows])
    with open(os.path.join(dirname, "small.yaml"), "w") as fh:
        fh.write("motions:\n"
                 "  - {file: small0.txt, weight: 0.5, play_speed: -0.7}\n"
                 "  - {file: small1.txt, weight: 0.2}\n"
                 "  - {file: small2.txt, weight: 1.0, play_speed: 1.5}\n")
    return os.path.join(dirname, "small.yaml")


def write_slerp_table(dirname: str) -> str:
    """One hand-made motion of six frames whose consecutive root rotations take slerp through its three branches: frames 0-1 identical
    (dot product exactly 1), 1-2 nearly parallel (1e-3 rad apart: s = 4.9e-4 < 0.001, c < 1), 2-3 a general pair with a NEGATIVE dot
    product (0.4 rad apart, the second quaternion negated), 3-4 a general pair with a positive one (both negated), 4-5 the same quaternion twice."""
    m = SY.table(1)[:6].copy()

    def rot(axis, ang):
        a = np.asarray(axis, dtype=np.float64)
        a = a / np.sqrt(a @ a)
        return np.concatenate([a * np.sin(ang / 2.0), [np.cos(ang / 2.0)]])
    q = [np.array([0.0, 0.0, 0.0, 1.0]), np.array([0.0, 0.0, 0.0, 1.0]), rot([0, 0, 1], 1e-3), -rot([1, 2, 3], 0.4), -rot([3, 1, 2], 0.7)]
    q.append(q[-1])
    m[:, 28:32] = np.stack(q)
    path = os.path.join(dirname, "slerp.txt")
    np.savetxt(path, m)
    return path


def queries(lib, seed=7, n_random=61):
    """(motion ids, times) that every test of the motion state shares: per motion t = 0, t = length, below zero, beyond the end, on a frame
    and just around one, then random ones."""
    ids, times = [], []
    for m in range(lib.num_motions()):
        L, dt = float(lib._motion_lengths[m]), abs(float(lib._motion_dt[m]))
        for t in (0.0, L, -0.003, -dt, L + 0.01, 3 * dt, np.nextafter(3 * dt, 0.0), np.nextafter(3 * dt, 1.0), 0.5 * L, L - 0.25 * dt):
            ids.append(m)
            times.append(t)
    rng = np.random.RandomState(seed)
    rm = rng.randint(0, lib.num_motions(), size=n_random)
    ids += list(rm)
    times += list(rng.uniform(-0.004, 1.0, size=n_random) * lib._motion_lengths[rm])
    return np.asarray(ids, dtype=np.int64), np.asarray(times, dtype=np.float64)


class HostTable:
    """device_table()'s tensors as numpy arrays"""

    def __init__(self, dt):
        for name in ("rows", "start", "num_frames", "length", "dt", "cum_weight"):
            setattr(self, name, getattr(dt, name).cpu().numpy())


def frame_blend(tab: HostTable, motion_ids, motion_times):
    """(row0, row1 into tab.rows, blend float64, frame0): phase = clip(t / length, 0, 1), frame0 = trunc(phase (frames - 1)), blend = (t - frame0 |dt|) / |dt|"""
    length, frames, dt = tab.length[motion_ids], tab.num_frames[motion_ids].astype(np.int64), np.abs(tab.dt[motion_ids])
    phase = np.clip(motion_times / length, 0.0, 1.0)
    i0 = (phase * (frames - 1)).astype(np.int64)
    i1 = np.minimum(i0 + 1, frames - 1)
    blend = (motion_times - i0 * dt) / dt
    start = tab.start[motion_ids].astype(np.int64)
    return start + i0, start + i1, blend, i0


def motion_state(tab: HostTable, motion_ids, motion_times):
    """get_motion_state from the float32 table: -> root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_pos (torch, CPU)"""
    motion_ids, motion_times = np.asarray(motion_ids), np.asarray(motion_times, dtype=np.float64)
    r0, r1, blend, _ = frame_blend(tab, motion_ids, motion_times)
    a, c = torch.from_numpy(tab.rows[r0]), torch.from_numpy(tab.rows[r1])
    b = torch.tensor(blend[:, np.newaxis], dtype=torch.float)
    root_pos = (1.0 - b) * a[:, RP] + b * c[:, RP]
    root_rot = ML.slerp(a[:, RR], c[:, RR], b)
    be = b.unsqueeze(-1)
    key_pos = (1.0 - be) * a[:, KEY].reshape(-1, 2, 3) + be * c[:, KEY].reshape(-1, 2, 3)
    return root_pos, root_rot, a[:, RV].clone(), a[:, RA].clone(), a[:, Q].clone(), a[:, QV].clone(), key_pos


def slerp_branch(tab: HostTable, motion_ids, motion_times):
    """per query: 0 identical (|c| >= 1), 1 nearly parallel (s < 0.001), 2 general; and whether the dot product is negative"""
    r0, r1, _, _ = frame_blend(tab, np.asarray(motion_ids), np.asarray(motion_times, dtype=np.float64))
    q0, q1 = torch.from_numpy(tab.rows[r0][:, RR]), torch.from_numpy(tab.rows[r1][:, RR])
    c = q0[:, 3] * q1[:, 3] + q0[:, 0] * q1[:, 0] + q0[:, 1] * q1[:, 1] + q0[:, 2] * q1[:, 2]
    ca = c.abs()
    s = torch.sqrt(1.0 - ca * ca)
    br = torch.where(ca >= 1, torch.zeros_like(c), torch.where(s < 0.001, torch.ones_like(c), torch.full_like(c, 2.0)))
    return br.numpy().astype(np.int64), (c < 0).numpy()


def device_start_draws(tab: HostTable, seed, num_envs, ctr, state_init, hybrid_prob):
    """The start dw_amp_reset_done_motion draws for EVERY env at draw counters ctr [N]: (kind int32, motion int32, time float64).  Block 0 of
    stream 15: word 0 -> reference start iff u < hybridInitProb (Hybrid), word 1 -> the first motion with u < cum_weight, word 2 -> time =
    float64(u) * length (0 for Start); u = float32(word >> 8) * 2^-24."""
    u = amp_draws.AmpDraws(seed, num_envs).uniform(ctr, DS_MOTION, [0, 1, 2])
    kind = (u[:, 0] < np.float32(hybrid_prob)).astype(np.int32) if state_init == "Hybrid" else np.ones(num_envs, np.int32)
    um = u[:, 1].astype(np.float64)
    motion = np.minimum((um[:, None] >= tab.cum_weight[None, :]).sum(axis=1), len(tab.cum_weight) - 1).astype(np.int32)
    time = np.zeros(num_envs) if state_init == "Start" else u[:, 2].astype(np.float64) * tab.length[motion]
    return kind, motion, time
