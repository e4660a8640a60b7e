#!/usr/bin/env python3
"""Cost of the stance inverse dynamics at --num-envs envs, --reps repetitions of every row, one process.
  kernel: microseconds per dwk_k_solve alone, from device events around replays of a captured chain of 100 launches (so that the host's
          launch rate does not bound it), on the buffers a real env holds after --warm-steps steps of small random actions: an all-on, a
          phase-mixed (the env's mocap rows spread over the gait: stance_from_phase) and an all-off stance, K = 2 and 4, with and without
          margins.  Beside them, measured the same way: dwi_k_solve with both feet, section 27's launch.
  today:  the path to the same phase-mixed tau_joint and force without this kernel, from section 27's entry point alone: three dwi_solve
          launches (the left foot's, the right foot's and both feet's tables) and torch.where by stance; with margins, the four words of
          every foot in torch as well.  In a captured chain like the kernel rows.
  step:   eager env.step() in milliseconds with stance_inverse_dynamics off / on / off / on ("auto": True); off is the parent commit's code
          path.
--launch-list: instead, the device events of 20 eager steps at 64 envs (torch.profiler) with the key absent and with "auto".
--tolerances: instead, on the CPU, the measured d per channel of tests/stance_inverse_dynamics_ref.py (float32 restatement against float64,
  4096 seeded states) and the largest solutions d was measured with."""
import argparse
import json
import os
import sys

SETS = {2: ["L_Foot_Link", "R_Foot_Link"], 4: ["L_Foot_Link", "R_Foot_Link", "L_Wrist2_Link", "R_Wrist2_Link"]}
KEY = "stance_inverse_dynamics"
POS = [0.0, 0.0, -0.09]


def kernel(n, warm_steps, launches, reps):
    import torch
    from _timing import DEV, make_env, chain_us
    from isaacgymdyros_amd import abi
    from isaacgymdyros_amd import contact_inverse_dynamics as IM
    from isaacgymdyros_amd import stance_inverse_dynamics as SM
    env = make_env(n, KEY, None)
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(warm_steps):
        env.step((torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * 0.05)
    abi.es_view(env._buf["env_state"], "mocap_data_idx")[:, 0] = (torch.arange(n, device=DEV, dtype=torch.int32) * 57) % 3600
    acc = torch.empty(n, 39, device=DEV).normal_(0.0, 20.0, generator=g)

    def row(name, what, us):
        print(json.dumps({"kernel": name, "num_envs": n, "outputs": what, "how": "captured chain of 100", "us_per_call": [round(u, 2) for u in us]}), flush=True)
    for K, bodies in SETS.items():
        for mg in (False, True):
            sd = SM.StanceInverseDynamics(env, {"contacts": [{"body": b, "pos": POS} for b in bodies], "contact_accel": False, "margins": mg, "base_residual": mg})
            sd.accel.copy_(acc)
            for name in ("all on", "phase-mixed", "all off"):
                sd.stance.fill_(0 if name == "all off" else 1)
                if name == "phase-mixed":
                    sd.stance_from_phase()
                what = "tau_joint + force + feasible%s, %d contacts, stance %s" % (" + margins + base_residual" if mg else "", K, name)
                row("dwk_k_solve", what, [chain_us(sd.refresh, launches) for _ in range(reps)])
            del sd
    both = IM.ContactInverseDynamics(env, {"contact_accel": False})
    both.accel.copy_(acc)
    row("dwi_k_solve", "tau_joint + force, 2 contacts (section 27)", [chain_us(both.refresh, launches) for _ in range(reps)])
    # today's path to the phase-mixed result: three launches of section 27 and torch.where by stance
    one = [IM.ContactInverseDynamics(env, {"contacts": [{"body": b, "pos": POS}], "contact_accel": False}) for b in SETS[2]]
    for o in one:
        o.accel.copy_(acc)
    sd = SM.StanceInverseDynamics(env, {"contact_accel": False})
    sd.accel.copy_(acc)
    st = sd.stance_from_phase().bool()
    l_only, r_only = (st[:, 0] & ~st[:, 1])[:, None], (st[:, 1] & ~st[:, 0])[:, None]
    zero6 = torch.zeros(n, 6, device=DEV)
    from isaacgymdyros_amd import body_states as BM
    bs = BM.BodyStates(env, {"bodies": SETS[2], "com": False})          # (the feet's rotations, for the margins in torch)
    so = torch.tensor(sd.soles, device=DEV)
    d = so[:, 0:3] - torch.tensor(sd.pos, device=DEV)

    def today(with_margins):
        both.refresh()
        one[0].refresh()
        one[1].refresh()
        tj = torch.where(l_only, one[0].tau_joint, torch.where(r_only, one[1].tau_joint, both.tau_joint))
        f = torch.where(l_only, torch.cat([one[0].force_all, zero6], 1), torch.where(r_only, torch.cat([zero6, one[1].force_all], 1), both.force_all))
        if not with_margins:
            return tj, f, None
        bs.refresh()
        q = bs.states[:, :, 3:7]
        x, y, z, w = q.unbind(-1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).view(n, 2, 3, 3)
        fw = f.view(n, 2, 6)
        fb, mb = torch.einsum("nkij,nki->nkj", R, fw[:, :, 0:3]), torch.einsum("nkij,nki->nkj", R, fw[:, :, 3:6])
        ms = mb - torch.cross(d[None].expand(n, 2, 3), fb, dim=-1)
        mgn = torch.stack([fb[..., 2], sd.friction * fb[..., 2] - torch.sqrt(fb[..., 0] ** 2 + fb[..., 1] ** 2), so[:, 3] * fb[..., 2] - ms[..., 1].abs(),
                           so[:, 4] * fb[..., 2] - ms[..., 0].abs()], -1) * st[:, :, None]
        return tj, f, mgn
    for mg in (False, True):
        what = "tau_joint + force%s, 2 contacts, stance phase-mixed" % (" + margins (torch, from the body-state tensor)" if mg else "")
        row("3 x dwi_k_solve + torch.where" + (" + dwb_k_states + torch" if mg else ""), what, [chain_us(lambda: today(mg), launches) for _ in range(reps)])
    tj, f, mgn = today(True)
    sd.refresh()
    torch.cuda.synchronize()
    print(json.dumps({"today's path against the launch": {"tau_joint": float((tj - sd.tau_joint).abs().max()), "force": float((f - sd.force_all).abs().max()),
                                                           "margins": float((mgn - sd.margins).abs().max()),
                                                           "largest force": float(sd.force_all.abs().max()), "feasible envs": int(sd.feasible.sum())}}), flush=True)
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
    import stance_inverse_dynamics_ref as SR
    for v in (0, 1):
        for K in (2, 4):
            for w in (None, SR.MOMENTS_10):
                for ref in (False, True):
                    d = SR.measured(v, K, w, ref)
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
