#!/usr/bin/env python3
"""Cost of the Jacobian and mass-matrix tensors at --num-envs envs.
  kernel: microseconds per dwj_k_jacobian / dwj_k_mass_matrix alone, from device events around replays of a captured chain of 100 launches (so
          that the host's launch rate does not bound it), on the buffers a real env holds after --warm-steps steps of small random actions: the
          Jacobian of all 38 bodies, of 3 bodies (head and both feet), the mass matrix with and without the COM Jacobian.  Beside each, in the
          same process and measured the same way, a device-to-device copy of the same number of output bytes: the yardstick for a store stream.
  step:   eager env.step() in milliseconds with jacobians off / on / off / on ("auto": True, every tensor); off is the parent commit's code path."""
import argparse
import json

import torch

from _timing import DEV, make_env, chain_us, step_ms


def kernel(n, warm_steps, launches):
    from isaacgymdyros_amd.jacobians import Jacobians
    env = make_env(n, "jacobians", None)
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(warm_steps):
        env.step((torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * 0.05)
    out = []
    feet = ["Head_Link", "L_Foot_Link", "R_Foot_Link"]
    for name, what, spec in (("dwj_k_jacobian", "38 bodies", {"mass_matrix": False}), ("dwj_k_jacobian", "3 bodies", {"bodies": feet, "mass_matrix": False}),
                             ("dwj_k_mass_matrix", "M + com_jacobian", {"jacobian": False, "com_jacobian": True}),
                             ("dwj_k_mass_matrix", "M", {"jacobian": False})):
        jc = Jacobians(env, spec)
        words = sum(t.numel() for t in (jc.jacobian, jc.mass_matrix, jc.com_jacobian) if t is not None)
        us = chain_us(jc.refresh, launches)
        src, dst = torch.rand(words, device=DEV), torch.empty(words, device=DEV)
        copy_us = chain_us(lambda: dst.copy_(src), launches)
        out.append({"kernel": name, "num_envs": n, "outputs": what, "output_bytes": 4 * words, "us_per_launch_in_a_captured_chain": us,
                    "GBps_stored": 4 * words / us * 1e-3, "d2d_copy_of_the_same_bytes_us": copy_us, "ratio_to_the_copy": us / copy_us})
        del jc, src, dst
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warm-steps", type=int, default=200)
    ap.add_argument("--launches", type=int, default=1000)
    a = ap.parse_args()
    for row in kernel(a.num_envs, a.warm_steps, a.launches):
        print(json.dumps(row), flush=True)
    feet = ["Head_Link", "L_Foot_Link", "R_Foot_Link"]
    for _ in range(a.rounds):
        for spec in (None, {"auto": True, "com_jacobian": True}, None, {"bodies": feet, "com_jacobian": True, "auto": True}):
            print(json.dumps(step_ms(a.num_envs, "jacobians", spec, 300, 50)), flush=True)


if __name__ == "__main__":
    main()
