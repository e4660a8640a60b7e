#!/usr/bin/env python3
"""Cost of TocabiAMPLower's episode statistics: milliseconds per eager step() + reset_done() at 16384 envs with amp_fused and
device draws, cfg sim.mi355.amp_episode_stats off and on in the same process, same seed and actions, each after a warm-up.  Run under
`rocprofv3 --kernel-trace --stats -- python tools/amp_episode_stats_time.py --only-on` for dwe_k_record's own time.

--lengths: no timing; the natural episode lengths of this robot under random torques (per-env action amplitude 0 .. 1, no time limit), as the
histogram tests/test_amp_episode_stats_gpu.py chose its episodeLength from, for the torch form, the fused form and the fused form with device
motion starts (stateInit Random on the synthetic tables of tests/amp_motion_synth.py)."""
import argparse
import json
import os
import sys
import tempfile

import torch

from _timing import DEV, ROOT, actions, loop_ms, make_amp_env

FUSED = {"amp_fused": True, "amp_hist_ring": True, "amp_device_draws": True}


def make(n, mi, episode_length=None, motion=False):
    env = {} if episode_length is None else {"episodeLength": episode_length}
    if motion:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import amp_motion_synth as SY
        env.update({"stateInit": "Random", "motion_file": SY.write(tempfile.mkdtemp(prefix="amp_synth_"))})
    return make_amp_env(n, mi, env)


def run(n, steps, warmup, on):
    env = make(n, dict(FUSED, amp_episode_stats=on))
    a = actions(n, 12, 0.5)
    out = {"amp_episode_stats": on, "num_envs": n,
           "ms_per_step_and_reset_done": loop_ms(lambda t: (env.reset_done(), env.step(a[t % 8])), steps, warmup)}
    if on:
        s = env.episode_stats.summary()
        out["episodes"], out["causes"], out["mean_length"] = s["episodes"], s["causes"], s["mean_length"]
    env.close()
    return out


def lengths(n, steps):
    for name, mi, motion in (("torch", {}, False), ("fused", FUSED, False), ("motion", dict(FUSED, amp_motion_device=True), True)):
        env = make(n, dict(mi, amp_episode_stats=True), episode_length=100000, motion=motion)
        g = torch.Generator(device=DEV).manual_seed(0)
        amp = torch.linspace(0.0, 1.0, n, device=DEV).unsqueeze(1)
        ended = []
        for _ in range(steps):
            env.reset_done()
            _o, _r, reset, _x = env.step((torch.rand(n, 12, generator=g, device=DEV) * 2 - 1) * amp)
            ended.append(env.progress_buf[reset.view(-1) != 0].cpu())
        ln = torch.cat(ended).float()
        s = env.episode_stats.summary()
        print(json.dumps({"form": name, "num_envs": n, "steps": steps, "episodes": int(ln.numel()), "median": float(ln.median()) if ln.numel() else None,
                          "hist_0_160_by_10": torch.histc(ln.clamp(max=159.0), bins=16, min=0, max=160).int().tolist(),
                          "cause_masks": s["cause_masks"], "contact_bodies": s["contact_bodies"]}), flush=True)
        env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--only-on", action="store_true")
    ap.add_argument("--lengths", action="store_true")
    a = ap.parse_args()
    if a.lengths:
        return lengths(256 if a.num_envs == 16384 else a.num_envs, 600 if a.steps == 1000 else a.steps)
    for on in ((True,) if a.only_on else (False, True, False, True)):
        print(json.dumps(run(a.num_envs, a.steps, a.warmup, on)), flush=True)


if __name__ == "__main__":
    main()
