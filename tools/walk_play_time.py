#!/usr/bin/env python3
"""Times the walk actor at play time -- dwp_play called directly, and through WalkPolicy.play with its host-side checks and allocations -- against
the rollout's forward of both nets (dwp_policy) and torch's actor forward (fp32, the torch backend's module) at the yaml's shapes (487
observations, 13 actions, units 256-256) and N = 1, 16, 32, 64, 65, 4096, 16384, with HIP events: the median of --reps timed calls after --warmup
untimed ones, every shape warmed up before it is timed.  Writes one JSON line per measurement to stdout and, with --out, the same lines to that
file (profiles/walk_play_time.json)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isaacgymdyros_amd import ppo_update as U          # noqa: E402
from isaacgymdyros_amd import walk_policy as WP         # noqa: E402


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
    ap.add_argument("--sizes", default="1,16,32,64,65,4096,16384")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    actor = WP.Actor().to(dev)
    hip = WP.WalkPolicy.from_module(actor, dev, backend="hip")
    tor = WP.WalkPolicy.from_module(actor, dev, backend="torch")
    g = torch.Generator(device=dev).manual_seed(0)
    s = torch.cuda.current_stream(dev).cuda_stream
    lines = []
    for n in [int(x) for x in args.sizes.split(",")]:
        obs, noise = torch.randn(n, U.IN, device=dev, generator=g), torch.randn(n, U.ACT, device=dev, generator=g)
        mu, val = torch.empty(n, U.ACT, device=dev), torch.empty(n, 1, device=dev)

        def policy():
            hip.api["policy"](obs.data_ptr(), hip.p.data_ptr(), hip.p32f.data_ptr(), n, mu.data_ptr(), val.data_ptr(), s)

        cl, w = torch.empty(n, U.ACT, device=dev), torch.empty(max(hip.work_floats(n), 1), device=dev)

        def play_raw():
            hip.api["play"](hip.p.data_ptr(), hip.p32f.data_ptr(), hip.logstd.data_ptr(), obs.data_ptr(), None, n, cl.data_ptr(), mu.data_ptr(),
                            w.data_ptr(), w.numel(), s)

        def torch_actor():
            with torch.no_grad():
                tor.net(obs)
        for what, fn in (("dwp_play", play_raw), ("walkpolicy_play", lambda: hip.play(obs)), ("dwp_play_stochastic", lambda: hip.play(obs, noise)),
                         ("dwp_policy", policy), ("torch_actor", torch_actor)):
            med, lo, hi = timed(fn, args.warmup, args.reps)
            lines.append(dict(what=what, envs=n, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4)))
            print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
