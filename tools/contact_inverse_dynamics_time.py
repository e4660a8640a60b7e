#!/usr/bin/env python3
"""Cost of the contact inverse dynamics at --num-envs envs, --reps repetitions of every row, one process.
  kernel: microseconds per dwi_k_solve alone, from device events around replays of a captured chain of 100 launches (so that the host's
          launch rate does not bound it), on the buffers a real env holds after --warm-steps steps of small random actions, for one, two and
          four contacts, with and without contact_accel.  Beside them, measured the same way: dwn_k_inverse_dynamics with tau alone, the
          floor (the same chain walk, records and subtree sums; none of the tail).
  today:  the path to the same tau_joint and force without this kernel, from the entry points of sections 24 and 26: dwn_inverse_dynamics
          for r, dwc_solve for jc alone, then torch for G = J_b' W^-1 J_b, its Cholesky, y, f = W^-1 J_b y and tau_joint = r[6:] - J_j' f
          (both feet, unit weights, no f_ref).  The batched LAPACK calls synchronise with the host on some back ends, so they cannot sit in
          a captured chain: these rows are eager calls between device events, and dwi_k_solve is measured that way once more beside them.
  step:   eager env.step() in milliseconds with contact_inverse_dynamics off / on / off / on ("auto": True); off is the parent commit's
          code path.
--launch-list: instead, the device events of 20 eager steps at 64 envs (torch.profiler) with the key absent and with "auto".
--tolerances: instead, on the CPU, the measured d per channel of tests/contact_inverse_dynamics_ref.py (float32 restatement against float64,
  4096 seeded states), the largest solutions d was measured with, and the largest cond(G)."""
import argparse
import json
import os
import sys

SETS = {1: ["L_Foot_Link"], 2: ["L_Foot_Link", "R_Foot_Link"], 4: ["L_Foot_Link", "R_Foot_Link", "L_Wrist2_Link", "R_Wrist2_Link"]}
KEY = "contact_inverse_dynamics"


def kernel(n, warm_steps, launches, reps):
    import torch
    from _timing import DEV, make_env, chain_us, eager_us
    from isaacgymdyros_amd import contact_dynamics as CM
    from isaacgymdyros_amd import contact_inverse_dynamics as IM
    from isaacgymdyros_amd.dynamics import Dynamics
    env = make_env(n, KEY, None)
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(warm_steps):
        env.step((torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * 0.05)

    def row(name, what, how, us):
        print(json.dumps({"kernel": name, "num_envs": n, "outputs": what, "how": how, "us_per_call": [round(u, 2) for u in us]}), flush=True)
    chained = "captured chain of 100"
    for K, bodies in SETS.items():
        for ca in (False, True):
            ci = IM.ContactInverseDynamics(env, {"contacts": [{"body": b, "pos": [0.0, 0.0, -0.09]} for b in bodies], "contact_accel": ca})
            ci.accel.normal_(0.0, 20.0)
            row("dwi_k_solve", "tau_joint + force%s, %d contact%s" % (" + contact_accel" if ca else "", K, "" if K == 1 else "s"), chained,
                [chain_us(ci.refresh, launches) for _ in range(reps)])
            del ci
    dyn = Dynamics(env, {"bias": False, "gravity": False, "inverse_dynamics": True})
    dyn.accel.normal_(0.0, 20.0)
    row("dwn_k_inverse_dynamics", "tau (the floor)", chained, [chain_us(dyn.inverse_dynamics, launches) for _ in range(reps)])
    # today's path to the same tau_joint and force, and the one launch beside it, as eager calls
    ci = IM.ContactInverseDynamics(env, {"contact_accel": False})
    ci.accel.copy_(dyn.accel)
    cd = CM.ContactDynamics(env, {"lambda": False})

    def today():
        r = dyn.inverse_dynamics()
        cd.refresh()
        Jb, Jj = cd.jc[:, :, 0:6], cd.jc[:, :, 6:]
        G = torch.bmm(Jb.transpose(1, 2), Jb)
        y = torch.cholesky_solve(r[:, 0:6].unsqueeze(2), torch.linalg.cholesky_ex(G, check_errors=False)[0])
        f = torch.bmm(Jb, y)
        return r[:, 6:] - torch.bmm(Jj.transpose(1, 2), f)[:, :, 0], f[:, :, 0]
    calls = max(launches // 50, 10)
    row("dwi_k_solve", "tau_joint + force, 2 contacts", "eager calls", [eager_us(ci.refresh, calls) for _ in range(reps)])
    row("dwn_k_inverse_dynamics + dwc_k_solve (jc) + torch (bmm, cholesky_ex, cholesky_solve)", "tau_joint + force, 2 contacts", "eager calls",
        [eager_us(today, calls) for _ in range(reps)])
    tj, f = today()
    ci.refresh()
    torch.cuda.synchronize()
    print(json.dumps({"today's path against the launch": {"tau_joint": float((tj - ci.tau_joint).abs().max()), "force": float((f - ci.force_all).abs().max()),
                                                           "largest force": float(ci.force_all.abs().max())}}), flush=True)
    env.close()


def launch_list():
    import torch
    from _timing import DEV, make_env
    from torch.profiler import ProfilerActivity, profile
    for spec in (None, {"auto": True}):
        env = make_env(64, KEY, spec)
        a = torch.zeros(64, 13, device=DEV)
        for _ in range(3):
            env.step(a)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(20):
                env.step(a)
            torch.cuda.synchronize()
        names = {}
        for ev in prof.events():
            if ev.device_type == torch.autograd.DeviceType.CUDA:
                k = ev.name.replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]
                names[k] = names.get(k, 0) + 1
        print(json.dumps({KEY: spec, "steps": 20, "device_events": sum(names.values()), "by_name": names}), flush=True)
        env.close()


def tolerances():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import contact_inverse_dynamics_ref as IR
    for v in (0, 1):
        for K in (1, 2, 4):
            for w in (None, IR.MOMENTS_10):
                for ref in (False, True):
                    d = IR.measured(v, K, w, ref)
                    print(json.dumps(dict({"vel_at_com": v, "contacts": K, "weights": "unit" if w is None else "moments 10 x", "f_ref": ref},
                                          **{k: float("%.3g" % x) for k, x in d.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm-steps", type=int, default=200)
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--launch-list", action="store_true")
    ap.add_argument("--tolerances", action="store_true")
    a = ap.parse_args()
    if a.tolerances:
        return tolerances()
    if a.launch_list:
        return launch_list()
    from _timing import step_ms
    kernel(a.num_envs, a.warm_steps, a.launches, a.reps)
    for _ in range(a.reps):
        for spec in (None, {"auto": True}):
            print(json.dumps(step_ms(a.num_envs, KEY, spec, 300, 50)), flush=True)


if __name__ == "__main__":
    main()
