#!/usr/bin/env python3
"""Cost of the bias-force, gravity, inverse-dynamics and momentum tensors at --num-envs envs.
  kernel: microseconds per dwn_k_inverse_dynamics alone, from device events around replays of a captured chain of 100 launches (so that the
          host's launch rate does not bound it), on the buffers a real env holds after --warm-steps steps of small random actions, for every
          output selection.  The output is 156 bytes per env and tensor, so a copy of the same bytes is no yardstick; beside them, in the same
          process and measured the same way, two other kernels: dwb_k_refresh restricted to the centre of mass (the same chain walk and the
          same 36 records: the floor for this shape of kernel) and dwj_k_mass_matrix (what M a costs today, before the batched product).
  step:   eager env.step() in milliseconds with dynamics off / on / off / on ("auto": True, bias + gravity + momentum); off is the parent
          commit's code path."""
import argparse
import json

import torch

from _timing import DEV, make_env, chain_us, step_ms


SELECTIONS = (("bias", {"gravity": False}), ("gravity", {"bias": False}), ("momentum", {"bias": False, "gravity": False, "momentum": True}),
              ("bias + gravity", {}), ("bias + gravity + momentum", {"momentum": True}),
              ("tau", {"bias": False, "gravity": False, "inverse_dynamics": True}),
              ("tau, no armature", {"bias": False, "gravity": False, "inverse_dynamics": True, "armature": False}))


def kernel(n, warm_steps, launches):
    from isaacgymdyros_amd.body_states import BodyStates
    from isaacgymdyros_amd.dynamics import Dynamics
    from isaacgymdyros_amd.jacobians import Jacobians
    env = make_env(n, "dynamics", None)
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(warm_steps):
        env.step((torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * 0.05)
    out = []

    def row(name, what, words, us):
        out.append({"kernel": name, "num_envs": n, "outputs": what, "output_bytes": 4 * words, "us_per_launch_in_a_captured_chain": us})
    for what, spec in SELECTIONS:
        dy = Dynamics(env, spec)
        words = sum(t.numel() for t in (dy.bias, dy.gravity, dy.momentum, dy.tau) if t is not None)
        if dy.tau is not None:
            dy.accel.normal_(0.0, 20.0)
            row("dwn_k_inverse_dynamics", what, words, chain_us(dy.inverse_dynamics, launches))
        else:
            row("dwn_k_inverse_dynamics", what, words, chain_us(dy.refresh, launches))
        del dy
    # all four in one launch: the entry point itself (the Python object makes tau a launch of its own)
    dy = Dynamics(env, {"inverse_dynamics": True, "momentum": True})
    args = list(dy._id_args)
    args[11], args[12], args[14] = dy.bias.data_ptr(), dy.gravity.data_ptr(), dy.momentum.data_ptr()
    dy._id_args = tuple(args)
    row("dwn_k_inverse_dynamics", "bias + gravity + tau + momentum", 3 * n * 39 + n * 6, chain_us(dy.inverse_dynamics, launches))
    del dy
    bs = BodyStates(env, {"bodies": [0]})
    args = list(bs._args)
    args[8] = None          # (no states: the centre of mass alone)
    bs._args = tuple(args)
    row("dwb_k_refresh", "com only", bs.com.numel(), chain_us(bs.refresh, launches))
    jc = Jacobians(env, {"jacobian": False})
    row("dwj_k_mass_matrix", "M", jc.mass_matrix.numel(), chain_us(jc.refresh, launches))
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warm-steps", type=int, default=200)
    ap.add_argument("--launches", type=int, default=1000)
    a = ap.parse_args()
    for r in kernel(a.num_envs, a.warm_steps, a.launches):
        print(json.dumps(r), flush=True)
    for _ in range(a.rounds):
        for spec in (None, {"momentum": True, "auto": True}, None, {"momentum": True, "auto": True}):
            print(json.dumps(step_ms(a.num_envs, "dynamics", spec, 300, 50)), flush=True)


if __name__ == "__main__":
    main()
