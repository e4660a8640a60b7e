#!/usr/bin/env python3
"""Times the AMP actor-critic (isaacgymdyros_amd/amp_policy.py) on one GPU with HIP events, both backends, at the yaml's shapes
(num_obs 468, 12 actions, units 512-512):
  act     one `act` call (normalisation, both nets, sampling, neglogp, value) at 4096 and 16384 envs
  update  one `update` (observation statistics, loss gradient, Adam) at the yaml's minibatch of 131 072 rows
  epoch   examples/amp_consumer.py --synthetic at 4096 envs with --policy_backend torch and hip: the total fps of its last epoch line
Prints one JSON line per measurement (median of --reps timed calls after --warmup; every shape is warmed up before it is timed)."""
import argparse
import json
import os
import subprocess
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


def line(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, default=468)
    ap.add_argument("--A", type=int, default=12)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=3, help="of the example run (0: skip it)")
    ap.add_argument("--only", default="", help="act, update or epoch: time only that (e.g. under a kernel trace)")
    args = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    D, A, B = args.D, args.A, args.rows
    obs = torch.randn(B, D, device=dev, generator=g)
    act = torch.randn(B, A, device=dev, generator=g) * 0.5
    old = torch.randn(B, device=dev, generator=g)
    adv, ret = torch.randn(B, device=dev, generator=g), torch.randn(B, device=dev, generator=g)
    for backend in ("hip", "torch"):
        pol = AP.AmpActorCritic(D, A, dev, backend=backend, seed=0)
        if args.only in ("", "act"):
            for n in (4096, 16384):
                o, nz = obs[:n].contiguous(), torch.randn(n, A, device=dev, generator=g)
                med, lo, hi = timed(lambda: pol.act(o, nz), args.warmup, args.reps)
                line(backend=backend, what="act", envs=n, D=D, A=A, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
        if args.only in ("", "update"):
            med, lo, hi = timed(lambda: pol.update(obs, act, old, adv, ret, lr=1e-6), args.warmup, args.reps)
            # the products of one update: forward 2 x (B D 512 + B 512 512), backward dW2 + dH1 + dW1 and the heads, 2 flops per multiply-add
            fl = 2 * 2 * B * (D * 512 + 512 * 512) + 2 * 2 * B * (512 * 512 * 2 + (D + 1) * 512) + 2 * B * 513 * (A + 1)
            line(backend=backend, what="update", rows=B, D=D, A=A, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                 gflop=round(fl / 1e9, 1), tflops_overall=round(fl / med / 1e9, 1))
    if args.epochs and args.only in ("", "epoch"):
        for backend in ("torch", "hip"):
            cmd = [sys.executable, os.path.join(ROOT, "examples", "amp_consumer.py"), "--synthetic", "--num_envs", "4096", "--epochs",
                   str(args.epochs), "--policy_backend", backend]
            r = subprocess.run(["timeout", "-k", "10", "900"] + cmd, capture_output=True, text=True, cwd=ROOT)
            eps = [ln for ln in r.stdout.splitlines() if ln.startswith("epoch ")]
            if r.returncode != 0 or not eps:
                line(backend=backend, what="epoch", error=(r.stdout + r.stderr)[-800:])
                raise SystemExit(1)
            f = eps[-1].split()
            line(backend=backend, what="epoch", envs=4096, horizon=32, epochs=args.epochs, step_fps_last=float(f[f.index("step") + 2]),
                 total_fps_last=float(f[f.index("total") + 2]), epoch_s_last=round(4096 * 32 / float(f[f.index("total") + 2]), 3))


if __name__ == "__main__":
    main()
