#!/usr/bin/env python3
"""Cost of the forward dynamics at --num-envs envs, --reps repetitions of every row, one process.
  kernel: microseconds per dwl_k_solve alone, from device events around replays of a captured chain of 100 launches (so that the host's
          launch rate does not bound it), on the buffers a real env holds after --warm-steps steps of small random actions: x alone with
          one right-hand side and with DWL_MAX_RHS, the factor, M^-1, and all three.  Beside them, measured the same way: dwj_k_mass_matrix
          (the same front end and a 100 MB store: the floor for this shape of kernel).
  today:  the path to the same x without this kernel: dwj_mass_matrix, then torch.linalg.cholesky_ex + torch.cholesky_solve, or
          torch.linalg.solve_ex, on the dense [N, 39, 39] batch.  The batched LAPACK calls synchronise with the host on some back ends, so they
          cannot sit in a captured chain: these rows are eager calls between device events, and dwl_k_solve is measured that way once more
          beside them.
  step:   eager env.step() in milliseconds with forward_dynamics off / on / off / on ("auto": True, factor + minv); off is the parent
          commit's code path."""
import argparse
import json

import torch

from _timing import DEV, make_env, chain_us, eager_us, step_ms


def kernel(n, warm_steps, launches, reps):
    from isaacgymdyros_amd import forward_dynamics as FM
    from isaacgymdyros_amd.jacobians import Jacobians
    env = make_env(n, "forward_dynamics", None)
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(warm_steps):
        env.step((torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * 0.05)

    def row(name, what, how, us):
        print(json.dumps({"kernel": name, "num_envs": n, "outputs": what, "how": how, "us_per_call": [round(u, 2) for u in us]}), flush=True)
    chained = "captured chain of 100"
    for what, spec, call in (("x, 1 right-hand side", {"rhs": 1}, "solve"), ("x, %d right-hand sides" % FM.MAX_RHS, {"rhs": FM.MAX_RHS}, "solve"),
                             ("factor", {"factor": True}, "refresh"), ("minv", {"minv": True}, "refresh")):
        fd = FM.ForwardDynamics(env, spec)
        fd.rhs.normal_(0.0, 50.0)
        row("dwl_k_solve", what, chained, [chain_us(getattr(fd, call), launches) for _ in range(reps)])
        del fd
    # all three in one launch: the entry point itself (the Python object makes x a launch of its own)
    fd = FM.ForwardDynamics(env, {"rhs": FM.MAX_RHS, "factor": True, "minv": True})
    fd.rhs.normal_(0.0, 50.0)
    args = list(fd._solve_args)
    args[11], args[12] = fd.factor.data_ptr(), fd.minv.data_ptr()
    fd._solve_args = tuple(args)
    row("dwl_k_solve", "x, %d right-hand sides + factor + minv" % FM.MAX_RHS, chained, [chain_us(fd.solve, launches) for _ in range(reps)])
    del fd
    jc = Jacobians(env, {"jacobian": False})
    row("dwj_k_mass_matrix", "M", chained, [chain_us(jc.refresh, launches) for _ in range(reps)])
    # today's path to the same x, and the one launch beside it, as eager calls
    fd = FM.ForwardDynamics(env, {"rhs": 1})
    fd.rhs.normal_(0.0, 50.0)
    b = fd.rhs.transpose(1, 2).contiguous()          # [N, 39, 1]

    def chol():
        M = jc.refresh_mass_matrix()
        return torch.cholesky_solve(b, torch.linalg.cholesky_ex(M, check_errors=False)[0])

    def lu():
        return torch.linalg.solve_ex(jc.refresh_mass_matrix(), b, check_errors=False)[0]
    calls = max(launches // 50, 10)
    row("dwl_k_solve", "x, 1 right-hand side", "eager calls", [eager_us(fd.solve, calls) for _ in range(reps)])
    row("dwj_k_mass_matrix + torch.linalg.cholesky_ex + torch.cholesky_solve", "x, 1 right-hand side", "eager calls", [eager_us(chol, calls) for _ in range(reps)])
    row("dwj_k_mass_matrix + torch.linalg.solve_ex", "x, 1 right-hand side", "eager calls", [eager_us(lu, calls) for _ in range(reps)])
    agree = float((fd.solve()[:, 0] - chol()[:, :, 0]).abs().max())
    print(json.dumps({"largest difference between dwl_solve's x and the dense Cholesky's": agree, "largest |x|": float(fd.x.abs().max())}), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm-steps", type=int, default=200)
    ap.add_argument("--launches", type=int, default=1000)
    a = ap.parse_args()
    kernel(a.num_envs, a.warm_steps, a.launches, a.reps)
    for _ in range(a.reps):
        for spec in (None, {"factor": True, "minv": True, "auto": True}):
            print(json.dumps(step_ms(a.num_envs, "forward_dynamics", spec, 300, 50)), flush=True)


if __name__ == "__main__":
    main()
