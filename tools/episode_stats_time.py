#!/usr/bin/env python3
"""Cost of the episode statistics: wall time per step() with cfg sim.mi355.episode_stats off and on, same seed and actions,
each after a warm-up.  Run under `rocprofv3 --kernel-trace --stats -- python tools/episode_stats_time.py --only-on` for dws_k_record's own time."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(n, steps, warmup, on):
    from isaacgymdyros_amd.config import default_cfg
    from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk
    cfg = default_cfg(n, "cuda:0")
    cfg["sim"]["mi355"]["episode_stats"] = on
    cfg["sim"]["mi355"]["alias_obs"] = True
    env = DyrosDynamicWalk(cfg, "cuda:0", 0, True)
    g = torch.Generator(device="cuda:0").manual_seed(0)
    acts = [torch.rand(n, 13, generator=g, device="cuda:0") * 2 - 1 for _ in range(8)]
    for t in range(warmup):
        env.step(acts[t % 8])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(steps):
        env.step(acts[t % 8])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    out = {"episode_stats": on, "num_envs": n, "ms_per_step": ms}
    if on:
        s = env.episode_stats.summary()
        out["episodes"], out["causes"] = s["episodes"], s["causes"]
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--only-on", action="store_true")
    a = ap.parse_args()
    for on in ((True,) if a.only_on else (False, True, False, True)):
        print(json.dumps(run(a.num_envs, a.steps, a.warmup, on)), flush=True)


if __name__ == "__main__":
    main()
