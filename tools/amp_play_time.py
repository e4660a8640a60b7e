#!/usr/bin/env python3
"""Times the play-time policy forward (AmpActorCritic.play, dwa_play) against the rollout forward (dwa_act, both nets) and the torch
backend's play at the yaml's shapes (num_obs 468, 12 actions, units 512-512) and N = 1, 64, 4096, 16384, with HIP events: the median of
--reps timed calls after --warmup untimed ones, every shape warmed up before it is timed.  Writes one JSON line per measurement to stdout and,
with --out, the same lines to that file (profiles/amp_play_time.json)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isaacgymdyros_amd import amp_policy as AP          # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, default=468)
    ap.add_argument("--A", type=int, default=12)
    ap.add_argument("--sizes", default="1,64,4096,16384")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    D, A = args.D, args.A
    hip = AP.AmpActorCritic(D, A, dev, backend="hip", seed=0)
    tor = AP.AmpActorCritic(D, A, dev, backend="torch", seed=0)
    lines = []
    for n in [int(x) for x in args.sizes.split(",")]:
        obs, noise = torch.randn(n, D, device=dev, generator=g), torch.randn(n, A, device=dev, generator=g)
        for what, fn in (("play", lambda: hip.play(obs)), ("play_stochastic", lambda: hip.play(obs, noise)),
                         ("act", lambda: hip.act(obs, noise)), ("torch_play", lambda: tor.play(obs))):
            med, lo, hi = timed(fn, args.warmup, args.reps)
            lines.append(dict(what=what, envs=n, D=D, A=A, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4)))
            print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
