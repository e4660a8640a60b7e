#!/usr/bin/env python3
"""Times the AMP discriminator (isaacgymdyros_amd/amp_disc.py) on one GPU with HIP events, both backends:
  reward  one `rewards` call over horizon 32 x 4096 envs = 131 072 rows of D = 68 (numAMPObsSteps 2)
  update  one `update` (statistics x 3, loss gradient, Adam) at the yaml's amp_minibatch_size: 131 072 agent, replay and demo rows
Prints one JSON line per measurement (median of --reps timed calls after --warmup)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isaacgymdyros_amd import amp_disc as AD          # noqa: E402


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
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--D", type=int, default=68)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(32, args.rows // 32, args.D, device=dev, generator=g)
    task = torch.randn(32, args.rows // 32, 1, device=dev, generator=g)
    a, r, d = (torch.randn(args.rows, args.D, device=dev, generator=g) + s for s in (-0.3, 0.0, 0.3))
    for backend in ("hip", "torch"):
        disc = AD.AmpDiscriminator(args.D, dev, backend=backend, seed=0)
        med, lo, hi = timed(lambda: disc.rewards(x, task), args.warmup, args.reps)
        print(json.dumps({"backend": backend, "what": "reward", "rows": args.rows, "D": args.D, "ms_median": round(med, 4), "ms_min": round(lo, 4),
                          "ms_max": round(hi, 4)}), flush=True)
        med, lo, hi = timed(lambda: disc.update(a, r, d, lr=1e-4), args.warmup, args.reps)
        print(json.dumps({"backend": backend, "what": "update", "rows_per_set": args.rows, "D": args.D, "ms_median": round(med, 4),
                          "ms_min": round(lo, 4), "ms_max": round(hi, 4)}), flush=True)


if __name__ == "__main__":
    main()
