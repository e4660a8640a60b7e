#!/usr/bin/env python3
"""Cost of the rigid-body state tensor at --num-envs envs.
  kernel: microseconds per dwb_k_refresh alone, from device events around replays of a captured chain of 100 launches (so that the host's
          launch rate does not bound it), on the buffers a real env holds after --warm-steps steps of small random actions: all 38 bodies plus
          the centre of mass, 3 bodies (head and both feet), and the centre of mass only.  Beside each, in the same process and measured the
          same way, a device-to-device copy of the same number of output bytes: the yardstick for a store stream.
  step:   eager env.step() in milliseconds with body_states off / on / off / on ("auto": True); off is the parent commit's code path."""
import argparse
import json

import torch

from _timing import DEV, make_env, chain_us, step_ms


def kernel(n, warm_steps, launches):
    from isaacgymdyros_amd.body_states import BodyStates
    env = make_env(n, "body_states", None)
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(warm_steps):
        env.step((torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * 0.05)
    out = []
    for what, spec in (("38 bodies + com", {}), ("3 bodies", {"bodies": ["Head_Link", "L_Foot_Link", "R_Foot_Link"], "com": False}),
                       ("com only", {"bodies": [0]})):
        bs = BodyStates(env, spec)
        if what == "com only":
            args = list(bs._args)
            args[8] = None          # (no states)
            bs._args = tuple(args)
        words = (0 if what == "com only" else bs.states.numel()) + (0 if bs.com is None else bs.com.numel())
        us = chain_us(bs.refresh, launches)
        src, dst = torch.rand(words, device=DEV), torch.empty(words, device=DEV)
        copy_us = chain_us(lambda: dst.copy_(src), launches)
        out.append({"kernel": "dwb_k_refresh", "num_envs": n, "outputs": what, "output_bytes": 4 * words, "us_per_launch_in_a_captured_chain": us,
                    "GBps_stored": 4 * words / us * 1e-3, "d2d_copy_of_the_same_bytes_us": copy_us, "ratio_to_the_copy": us / copy_us})
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warm-steps", type=int, default=200)
    a = ap.parse_args()
    for row in kernel(a.num_envs, a.warm_steps, 2000):
        print(json.dumps(row), flush=True)
    for _ in range(a.rounds):
        for spec in (None, {"auto": True}):
            print(json.dumps(step_ms(a.num_envs, "body_states", spec, 500, 50, flag=True)), flush=True)


if __name__ == "__main__":
    main()
