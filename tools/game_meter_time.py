#!/usr/bin/env python3
"""Cost of the learners' episode-return meter at --num-envs envs: microseconds per dwm_k_record alone for C = 1 and
C = 16 columns (device events around replays of a captured chain of 100 launches, so that the host's launch rate does not bound it; the
inputs are a step's worth of rewards with a done probability of 1 / 500), and config 3 -- the fused update behind a captured rollout,
examples/ppo_consumer.py train(graph_rollout=True, fused_update=True) -- total_fps with game_meter off and on, interleaved in one process,
the first epoch of every run left out.  Run under `rocprofv3 --kernel-trace --stats -- python tools/game_meter_time.py --only-on` for the
kernel's own time within a rollout."""
import argparse
import importlib.util
import json
import os

import torch

from _timing import DEV, ROOT, chain_us


def kernel(n, cols, launches):
    from isaacgymdyros_amd.game_meter import GameMeter
    g = torch.Generator(device=DEV).manual_seed(0)
    m = GameMeter(n, DEV, cols=cols, games_to_track=100)
    rew = torch.randn(n, generator=g, device=DEV)
    stacked = torch.randn(n, 15, generator=g, device=DEV)
    done = (torch.rand(n, generator=g, device=DEV) < 1.0 / 500).to(torch.int64)
    args = (rew, done, stacked if cols > 1 else None)
    us = chain_us(lambda: m.record(*args), launches)
    # bytes: every column of cur read and written, the increments and the flags read
    moved = n * (8 * (cols + 1) + 4 * cols + 8)
    s = m.summary()
    return {"kernel": "dwm_k_record", "num_envs": n, "cols": cols, "us_per_launch_in_a_captured_chain": us, "bytes": moved, "GB_per_s": moved / us / 1e3,
            "games": s["games"], "done_per_launch": int(done.sum())}


def consumer(n, epochs, on):
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(ROOT, "examples", "ppo_consumer.py"))
    ppo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ppo)
    st = ppo.train(num_envs=n, epochs=epochs, device=DEV, graph_rollout=True, fused_update=True, game_meter=on, log=lambda s: None)
    fps = sorted(s["total_fps"] for s in st[1:])
    out = {"config": 3, "game_meter": on, "num_envs": n, "epochs_timed": len(fps), "total_fps_median": fps[len(fps) // 2], "total_fps_best": fps[-1]}
    if on:
        out["games"] = st[-1]["game_meter"]["games"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only-on", action="store_true")
    a = ap.parse_args()
    if a.only_on:
        print(json.dumps(consumer(a.num_envs, a.epochs, True)), flush=True)
        return
    for cols in (1, 16):
        print(json.dumps(kernel(a.num_envs, cols, 2000)), flush=True)
    for _ in range(a.rounds):
        for on in (False, True):
            print(json.dumps(consumer(a.num_envs, a.epochs, on)), flush=True)


if __name__ == "__main__":
    main()
