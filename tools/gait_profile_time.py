#!/usr/bin/env python3
"""Cost of the gait profile at --num-envs envs.
  kernel:   microseconds per dwg_k_record alone, from device events around replays of a captured chain of 100 launches (so that the host's launch
            rate does not bound it), on the buffers a real env holds after --warm-steps steps of small random actions; once as the env left
            them (every env started at mocap row 0 or 1800, so few bins are occupied and their rows are contended) and once with the
            mocap index of a copy of env_state spread uniformly over the cycle, for 72 and 144 bins
  step:     eager env.step() in milliseconds with the profile off and on
  consumer: config 3 -- the fused update behind a captured rollout, examples/ppo_consumer.py train(graph_rollout=True, fused_update=True) --
            total_fps with gait_profile off and on, interleaved in one process, the first epoch of every run left out; off is the parent
            commit's code path (no launch is added)."""
import argparse
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from _timing import DEV, make_env, chain_us, step_ms


def kernel(n, bins, warm_steps, launches):
    from isaacgymdyros_amd import abi, cbind
    env = make_env(n, "gait_profile", {"bins": bins})
    gp = env.gait_profile
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(warm_steps):
        env.step((torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * 0.05)
    out = []
    idx = abi.es_view(env._buf["env_state"], "mocap_data_idx").reshape(-1)
    for spread in (False, True):
        args = list(gp._record_args)
        if spread:
            es = env._buf["env_state"].clone()
            abi.es_view(es, "mocap_data_idx").reshape(-1).copy_(torch.randint(0, 3599, (n,), generator=g, device=DEV, dtype=torch.int32))
            args[7] = es.data_ptr()
            idx = abi.es_view(es, "mocap_data_idx").reshape(-1)
        gp.reset_totals()
        us = chain_us(lambda: cbind.check(gp.api, gp.api["record"](*args, gp._stream())), launches)
        s = gp.summary()
        out.append({"kernel": "dwg_k_record", "num_envs": n, "bins": bins, "mocap_idx": "spread uniformly" if spread else "as the env left it",
                    "bins_occupied": int((torch.bincount((idx // (3600 // bins)).long(), minlength=bins) > 0).sum()),
                    "us_per_launch_in_a_captured_chain": us, "recorded_per_launch": s["recorded"] / (launches + 101),
                    "skipped_terminal_per_launch": s["skipped_terminal"] / (launches + 101)})
    env.close()
    return out


def consumer(n, epochs, on):
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(ROOT, "examples", "ppo_consumer.py"))
    ppo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ppo)
    st = ppo.train(num_envs=n, epochs=epochs, device=DEV, graph_rollout=True, fused_update=True, gait_profile=on or None, log=lambda s: None)
    fps = sorted(s["total_fps"] for s in st[1:])
    out = {"config": 3, "gait_profile": on, "num_envs": n, "epochs_timed": len(fps), "total_fps_median": fps[len(fps) // 2], "total_fps_best": fps[-1]}
    if on:
        g = st[-1]["gait_profile"]
        out.update(recorded=g["recorded"], skipped_terminal=g["skipped_terminal"], paid_fraction_DSP=float(g["windows"]["DSP"]["paid_fraction"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warm-steps", type=int, default=200)
    a = ap.parse_args()
    for bins in (72, 144):
        for row in kernel(a.num_envs, bins, a.warm_steps, 2000):
            print(json.dumps(row), flush=True)
    for _ in range(a.rounds):
        for profile in (None, {"bins": 72}):
            print(json.dumps(step_ms(a.num_envs, "gait_profile", profile, 500, 50, flag=True)), flush=True)
    for _ in range(a.rounds):
        for on in (False, True):
            print(json.dumps(consumer(a.num_envs, a.epochs, on)), flush=True)


if __name__ == "__main__":
    main()
