#!/usr/bin/env python3
"""Cost of the contact-consistent dynamics at --num-envs envs, --reps repetitions of every row, one process.
  kernel: microseconds per dwc_k_solve alone, from device events around replays of a captured chain of 100 launches (so that the host's
          launch rate does not bound it), on the buffers a real env holds after --warm-steps steps of small random actions, per output
          selection, both feet planted.  Beside them, measured the same way: dwl_k_solve with DWL_MAX_RHS right-hand sides, the floor (the
          same front end, factor and sweeps, a third of the columns).
  today:  the path to the same accel and force without this kernel, from the shipped entry points: dwj_jacobian for the contact bodies,
          dwl_solve for Y = M^-1 J_c' and x0 (13 columns: two launches), then torch for A = J_c Y, its Cholesky, A f = -Jd_c nu - J_c x0 and
          accel = x0 + Y f.  dwj_jacobian's rows are taken at the bodies' own points, not shifted to the contact points, and Jd_c nu, which no
          shipped entry point gives, is read from a buffer filled beforehand: both omissions favour today's path.  The batched LAPACK calls
          synchronise with the host on some back ends, so they cannot sit in a captured chain: these rows are eager calls between device
          events, and dwc_k_solve is measured that way once more beside them.
  step:   eager env.step() in milliseconds with contact_dynamics off / on / off / on ("auto": True, the default outputs); off is the parent
          commit's code path."""
import argparse
import json

import torch

from _timing import DEV, make_env, chain_us, eager_us, step_ms
FEET = ["L_Foot_Link", "R_Foot_Link"]


def kernel(n, warm_steps, launches, reps):
    from isaacgymdyros_amd import contact_dynamics as CM
    from isaacgymdyros_amd import forward_dynamics as FM
    from isaacgymdyros_amd.jacobians import Jacobians
    env = make_env(n, "contact_dynamics", None)
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(warm_steps):
        env.step((torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * 0.05)

    def row(name, what, how, us):
        print(json.dumps({"kernel": name, "num_envs": n, "outputs": what, "how": how, "us_per_call": [round(u, 2) for u in us]}), flush=True)
    chained = "captured chain of 100"
    off = {"jacobian": False, "lambda": False}
    for what, spec, call in (("jc + jdnu", {"lambda": False}, "refresh"), ("lambda", dict(off, **{"lambda": True}), "refresh"),
                             ("lambda_inv", dict(off, lambda_inv=True), "refresh"), ("minv_jt", dict(off, minv_jt=True), "refresh"),
                             ("jc + jdnu + lambda (the default)", {}, "refresh"),
                             ("jc + jdnu + lambda + lambda_inv + minv_jt", {"lambda_inv": True, "minv_jt": True}, "refresh"),
                             ("accel + force, 1 right-hand side", dict(off, rhs=1), "solve"),
                             ("accel + force, %d right-hand sides" % CM.MAX_RHS, dict(off, rhs=CM.MAX_RHS), "solve")):
        cd = CM.ContactDynamics(env, spec)
        cd.rhs.normal_(0.0, 50.0)
        row("dwc_k_solve", what, chained, [chain_us(getattr(cd, call), launches) for _ in range(reps)])
        del cd
    fd8 = FM.ForwardDynamics(env, {"rhs": FM.MAX_RHS})
    fd8.rhs.normal_(0.0, 50.0)
    row("dwl_k_solve", "x, %d right-hand sides (the floor)" % FM.MAX_RHS, chained, [chain_us(fd8.solve, launches) for _ in range(reps)])
    # today's path to the same accel and force, and the one launch beside it, as eager calls
    cd = CM.ContactDynamics(env, {"rhs": 1})
    cd.rhs.normal_(0.0, 50.0)
    cd.refresh()
    jac = Jacobians(env, {"bodies": FEET, "mass_matrix": False})
    fd5 = FM.ForwardDynamics(env, {"rhs": 5})
    jd = cd.jdnu.clone()

    def today():
        J = jac.refresh_jacobian().reshape(n, 12, 39)
        fd8.rhs.copy_(J[:, 0:8])
        fd5.rhs[:, 0:4].copy_(J[:, 8:12])
        fd5.rhs[:, 4].copy_(cd.rhs[:, 0])
        y8, y5 = fd8.solve(), fd5.solve()
        Y, x0 = torch.cat([y8, y5[:, 0:4]], 1), y5[:, 4]                  # [N, 12, 39], [N, 39]
        A = torch.bmm(J, Y.transpose(1, 2))
        gr = (-jd - torch.bmm(J, x0.unsqueeze(2))[:, :, 0]).unsqueeze(2)
        f = torch.cholesky_solve(gr, torch.linalg.cholesky_ex(A, check_errors=False)[0])
        return x0 + torch.bmm(Y.transpose(1, 2), f)[:, :, 0], f[:, :, 0]
    calls = max(launches // 50, 10)
    row("dwc_k_solve", "accel + force, 1 right-hand side", "eager calls", [eager_us(cd.solve, calls) for _ in range(reps)])
    row("dwj_k_jacobian + 2 dwl_k_solve + torch (bmm, cholesky_ex, cholesky_solve)", "accel + force, 1 right-hand side", "eager calls",
        [eager_us(today, calls) for _ in range(reps)])
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
        for spec in (None, {"auto": True}):
            print(json.dumps(step_ms(a.num_envs, "contact_dynamics", spec, 300, 50)), flush=True)


if __name__ == "__main__":
    main()
