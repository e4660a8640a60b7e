#!/usr/bin/env python3
"""Plays a DyrosDynamicWalk PPO policy from a checkpoint, as the reference's play path does (paths relative to
python/IsaacGymEnvs/isaacgymenvs/learning/rl_games_custom): restore, the text export TOCABI's controller loads (torch_runner_dyros.py:133-150:
every model tensor as <name with . -> _>.txt), then rl_games' PpoPlayerContinuous loop, restated here as examples/amp_player.py restates
CommonPlayer (rl_games is not part of the reference's checkout): the policy's action, env.step (which resets finished envs itself), the reward
and the steps summed per env; on done envs `reward: ... steps: ...` (the means over the envs done at that step), at the end
`av reward: ... av steps: ...`.

The action is WalkPolicy.play (isaacgymdyros_amd/walk_policy.py): the actor in eval mode, deterministic clamp(mu, -1, 1) -- rescale_actions is the
identity on this task's +-1 action space (tasks/base/vec_task.py:95) -- or, with --stochastic, clamp(mu + exp(sigma) noise, -1, 1).  On
--policy-backend hip that is dwp_play.  An episode is 32 s at 4 ms per policy step (8000 steps); --max-steps defaults to 10000, so every game can
end on its own.

--trace-dir DIR turns the on-GPU run trace on (isaacgymdyros_amd/run_trace.py): the last --trace-depth steps of envs
0 .. --trace-envs - 1.  With --trace-hold fall (the default) or reset a slot freezes at the step that ends its episode; after each round of games
the held slots are written to DIR/fall_env<id>_<n>.npz and armed again, and the count is printed at the end.  With never the rings are written
once at the end, as DIR/ring_env<id>.npz.

--gait-report turns the on-GPU gait profile on (isaacgymdyros_amd/gait_profile.py) and prints, after playing, the mean
vertical sole force per foot in the reward's three gait windows beside the mocap force columns, and how often foot_contact_reward was paid.
--gait-dir DIR also writes the per-bin profile as DIR/gait_profile.npz and DIR/gait_profile.txt; --gait-bins sets the number of phase bins.

--bodies-dir DIR turns the rigid-body state tensor on (isaacgymdyros_amd/body_states.py) and records envs
0 .. --bodies-envs - 1 at every step; at the end it writes DIR/bodies_env<id>.npz with names, parents, dt, states [T, 38, 13] (position,
quaternion xyzw, linear and angular velocity of every body in the world frame) and com [T, 7]: the file an external viewer reads.

--sensors-dir DIR turns the foot force-torque sensors on (isaacgymdyros_amd/force_sensors.py) and records envs
0 .. --sensors-envs - 1 at every step; at the end it writes DIR/sensors_env<id>.npz with names, dt, sensors [T, S, 6] (force then torque of the
ground on each foot, in the sensor frame), cop [T, 2, 4] (x, y in the foot frame, Fz, loaded corners) and zmp [T, 4].

--scan-dir DIR turns the terrain height scan on (isaacgymdyros_amd/height_scan.py) and records envs
0 .. --scan-envs - 1 at every step; at the end it writes DIR/scan_env<id>.npz with grid [P, 2], names, dt, heights [T, P] (the ground around
the base, the reference's get_heights), probe_pos [T, B, 3] and clearance [T, B] (the sole corners and their height over the ground).

--dynamics-dir DIR turns the Jacobian and mass-matrix tensors on (isaacgymdyros_amd/jacobians.py) and records envs
0 .. --dynamics-envs - 1 at every step; at the end it writes DIR/dynamics_env<id>.npz with names, dof_names, dt, jacobian [T, 3, 6, 39] (head and
both feet; rows linear then angular, columns the root's linear and angular velocity then the 33 DoFs), mass_matrix [T, 39, 39] and
com_jacobian [T, 3, 39].  With --dynamics-forces it also turns the bias-force, gravity and momentum tensors on (isaacgymdyros_amd/dynamics.py,
DESIGN.md section 24) and adds bias [T, 39], gravity [T, 39] and momentum [T, 6] to each file; without the flag the files are unchanged.  With --dynamics-accel it
turns the forward dynamics on (isaacgymdyros_amd/forward_dynamics.py) and adds minv [T, 39, 39] = M^-1 and
accel_zero_torque [T, 39] = M^-1 (-h), the acceleration of the unactuated robot in free flight; without the flag the files are unchanged.  With --dynamics-contact it turns the
contact-consistent dynamics on (isaacgymdyros_amd/contact_dynamics.py) with both feet planted and adds contact_jacobian
[T, 12, 39], contact_lambda [T, 12, 12] (the contact-space inertia) and contact_force_zero_torque [T, 2, 6], the ground reaction (force, then
moment about the sensor frame's origin, world axes) the unactuated robot with planted feet would get; without the flag the files are unchanged.
With --dynamics-inverse it turns the contact inverse dynamics on (isaacgymdyros_amd/contact_inverse_dynamics.py) with both
feet as contacts and adds hold_torque [T, 33] and hold_force [T, 2, 6]: the joint torques and the foot wrenches that would keep nu_dot = 0 at
each played state; without the flag the files are unchanged.
With --dynamics-stance it turns the stance inverse dynamics on (isaacgymdyros_amd/stance_inverse_dynamics.py) and adds
stance [T, 2] (which foot the gait's phase loads), stance_torque [T, 33], stance_force [T, 2, 6] and stance_margins [T, 2, 4]: the same
question under the phase's stance, and how far each loaded sole is from what it can deliver; without the flag the files are unchanged.
With --dynamics-ik it turns the inverse kinematics on (isaacgymdyros_amd/inverse_kinematics.py) and, at each played step,
solves both feet's played poses from the model's initial joint angles; it adds ik_q [T, 33], ik_err [T, 2] (the largest position and
orientation error left) and ik_converged [T]; without the flag the files are unchanged.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isaacgymdyros_amd import ppo_checkpoint as PK          # noqa: E402


def drain_held(trace, directory: str, n: int) -> int:
    """Writes every held slot's ring to directory/fall_env<id>_<n>.npz, arms those slots again; returns the new file count."""
    from isaacgymdyros_amd.run_trace import write_npz
    for f in trace.drain():
        write_npz(os.path.join(directory, "fall_env%d_%d.npz" % (f["env_id"], n)), f)
        n += 1
    return n


def run(args):
    from isaacgymdyros_amd.config import default_cfg
    from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk
    dev = torch.device(args.device)
    cfg = default_cfg(args.num_envs, args.device)
    if args.nominal:
        # the guide's "nominal environment": no domain randomisation and no pushes.  The encoder noise and biases of the observations have no
        # switch in the reference, so they stay on
        cfg["task"]["randomize"] = False
        cfg["env"]["perturbation"] = False
        print("nominal environment: task.randomize False, env.perturbation False (encoder noise and biases stay on: the reference has no switch "
              "for them)", flush=True)
    if args.episode_length is not None:
        cfg["env"]["episodeLength"] = float(args.episode_length)
    if args.report:
        cfg["sim"]["mi355"]["episode_stats"] = True
    if args.trace_dir:
        cfg["sim"]["mi355"]["run_trace"] = {"env_ids": min(args.trace_envs, args.num_envs), "depth": args.trace_depth, "hold": args.trace_hold}
        os.makedirs(args.trace_dir, exist_ok=True)
    if args.gait_report or args.gait_dir:
        cfg["sim"]["mi355"]["gait_profile"] = {"bins": args.gait_bins}
    if args.bodies_dir:
        cfg["sim"]["mi355"]["body_states"] = {"auto": True}
        os.makedirs(args.bodies_dir, exist_ok=True)
    if args.sensors_dir:
        cfg["sim"]["mi355"]["force_sensors"] = {"auto": True}
        os.makedirs(args.sensors_dir, exist_ok=True)
    if args.scan_dir:
        cfg["sim"]["mi355"]["height_scan"] = {"auto": True}
        os.makedirs(args.scan_dir, exist_ok=True)
    if args.dynamics_dir:
        cfg["sim"]["mi355"]["jacobians"] = {"bodies": ["Head_Link", "L_Foot_Link", "R_Foot_Link"], "com_jacobian": True, "auto": True}
        if args.dynamics_forces:
            cfg["sim"]["mi355"]["dynamics"] = {"momentum": True, "auto": True}
        if args.dynamics_accel:
            cfg["sim"]["mi355"]["forward_dynamics"] = {"minv": True, "auto": True}
        if args.dynamics_contact:
            cfg["sim"]["mi355"]["contact_dynamics"] = {"auto": True}
        if args.dynamics_inverse:
            cfg["sim"]["mi355"]["contact_inverse_dynamics"] = {"contact_accel": False, "auto": True}
        if args.dynamics_stance:
            cfg["sim"]["mi355"]["stance_inverse_dynamics"] = {"contact_accel": False, "base_residual": False}
        if args.dynamics_ik:
            cfg["sim"]["mi355"]["inverse_kinematics"] = True
        os.makedirs(args.dynamics_dir, exist_ok=True)
    env = DyrosDynamicWalk(cfg, args.device, 0, True)
    traces_written = 0
    bodies_k = min(max(args.bodies_envs, 1), args.num_envs) if args.bodies_dir else 0
    if bodies_k:          # (preallocated: a step adds two device-to-device copies and no host sync)
        rec_states = torch.zeros(args.max_steps, bodies_k, 38, 13, device=dev)
        rec_com = torch.zeros(args.max_steps, bodies_k, 7, device=dev)
    sensors_k = min(max(args.sensors_envs, 1), args.num_envs) if args.sensors_dir else 0
    if sensors_k:
        rec_sen = torch.zeros(args.max_steps, sensors_k, len(env.force_sensors.names), 6, device=dev)
        rec_cop = torch.zeros(args.max_steps, sensors_k, 2, 4, device=dev)
        rec_zmp = torch.zeros(args.max_steps, sensors_k, 4, device=dev)
    scan_k = min(max(args.scan_envs, 1), args.num_envs) if args.scan_dir else 0
    if scan_k:
        hsc = env.height_scan
        rec_hts = torch.zeros(args.max_steps, scan_k, hsc.heights.shape[1], device=dev)
        rec_ppos = torch.zeros(args.max_steps, scan_k, len(hsc.names), 3, device=dev)
        rec_clr = torch.zeros(args.max_steps, scan_k, len(hsc.names), device=dev)
    dynamics_k = min(max(args.dynamics_envs, 1), args.num_envs) if args.dynamics_dir else 0
    if dynamics_k:
        rec_jac = torch.zeros(args.max_steps, dynamics_k, 3, 6, 39, device=dev)
        rec_mm = torch.zeros(args.max_steps, dynamics_k, 39, 39, device=dev)
        rec_cj = torch.zeros(args.max_steps, dynamics_k, 3, 39, device=dev)
    forces = bool(dynamics_k and args.dynamics_forces)
    if forces:
        rec_bias = torch.zeros(args.max_steps, dynamics_k, 39, device=dev)
        rec_grav = torch.zeros(args.max_steps, dynamics_k, 39, device=dev)
        rec_mom = torch.zeros(args.max_steps, dynamics_k, 6, device=dev)
    accel = bool(dynamics_k and args.dynamics_accel)
    if accel:
        rec_minv = torch.zeros(args.max_steps, dynamics_k, 39, 39, device=dev)
        rec_acc = torch.zeros(args.max_steps, dynamics_k, 39, device=dev)
    contact = bool(dynamics_k and args.dynamics_contact)
    if contact:
        rec_cjac = torch.zeros(args.max_steps, dynamics_k, 12, 39, device=dev)
        rec_clam = torch.zeros(args.max_steps, dynamics_k, 12, 12, device=dev)
        rec_cf = torch.zeros(args.max_steps, dynamics_k, 2, 6, device=dev)
    inverse = bool(dynamics_k and args.dynamics_inverse)
    if inverse:
        rec_ht = torch.zeros(args.max_steps, dynamics_k, 33, device=dev)
        rec_hf = torch.zeros(args.max_steps, dynamics_k, 2, 6, device=dev)
    stance = bool(dynamics_k and args.dynamics_stance)
    if stance:
        rec_st = torch.zeros(args.max_steps, dynamics_k, 2, dtype=torch.uint8, device=dev)
        rec_stt = torch.zeros(args.max_steps, dynamics_k, 33, device=dev)
        rec_stf = torch.zeros(args.max_steps, dynamics_k, 2, 6, device=dev)
        rec_stm = torch.zeros(args.max_steps, dynamics_k, 2, 4, device=dev)
    ik = bool(dynamics_k and args.dynamics_ik)
    if ik:
        rec_ikq = torch.zeros(args.max_steps, dynamics_k, 33, device=dev)
        rec_ike = torch.zeros(args.max_steps, dynamics_k, 2, device=dev)
        rec_ikc = torch.zeros(args.max_steps, dynamics_k, dtype=torch.uint8, device=dev)
    played = 0
    ck = PK.load(args.checkpoint)
    n_obs, n_act = int(ck["model"][PK.PREFIX + "actor_mlp.0.weight"].shape[1]), int(ck["model"][PK.PREFIX + "mu.weight"].shape[0])
    if (n_obs, n_act) != (env.num_obs, env.num_acts):
        raise SystemExit("checkpoint: %d observations / %d actions, the task has %d / %d" % (n_obs, n_act, env.num_obs, env.num_acts))
    if args.export_dir:
        PK.export_txt(ck, args.export_dir)
    pol = PK.load_policy(ck, dev, backend=args.policy_backend)
    N, games_played, sum_rewards, sum_steps = env.num_envs, 0, 0.0, 0.0
    obs = env.reset()["obs"]
    cr = torch.zeros(N, device=dev)
    steps = torch.zeros(N, device=dev)
    for _n in range(args.max_steps):
        noise = torch.randn(N, n_act, device=dev) if args.stochastic else None
        action, _mu = pol.play(obs.contiguous(), noise)
        o, r, done, _info = env.step(action)
        obs = o["obs"]
        if bodies_k:
            rec_states[_n].copy_(env.body_states.states[:bodies_k])
            rec_com[_n].copy_(env.body_states.com[:bodies_k])
        if sensors_k:
            rec_sen[_n].copy_(env.force_sensors.sensors[:sensors_k])
            rec_cop[_n].copy_(env.force_sensors.cop[:sensors_k])
            rec_zmp[_n].copy_(env.force_sensors.zmp[:sensors_k])
        if scan_k:
            rec_hts[_n].copy_(hsc.heights[:scan_k])
            rec_ppos[_n].copy_(hsc.probe_pos[:scan_k])
            rec_clr[_n].copy_(hsc.clearance[:scan_k])
        if dynamics_k:
            rec_jac[_n].copy_(env.jacobians.jacobian[:dynamics_k])
            rec_mm[_n].copy_(env.jacobians.mass_matrix[:dynamics_k])
            rec_cj[_n].copy_(env.jacobians.com_jacobian[:dynamics_k])
        if forces:
            rec_bias[_n].copy_(env.dynamics.bias[:dynamics_k])
            rec_grav[_n].copy_(env.dynamics.gravity[:dynamics_k])
            rec_mom[_n].copy_(env.dynamics.momentum[:dynamics_k])
        if accel:
            rec_minv[_n].copy_(env.forward_dynamics.minv[:dynamics_k])
            rec_acc[_n].copy_(env.forward_dynamics.forward_dynamics()[:dynamics_k])
        if contact:
            env.contact_dynamics.forward_dynamics()
            rec_cjac[_n].copy_(env.contact_dynamics.jc[:dynamics_k])
            rec_clam[_n].copy_(env.contact_dynamics.lambda_[:dynamics_k])
            rec_cf[_n].copy_(env.contact_dynamics.force[:dynamics_k])
        if inverse:          # (accel stays zero: what the auto refresh left are the holding torques and wrenches)
            rec_ht[_n].copy_(env.contact_inverse_dynamics.tau_joint[:dynamics_k])
            rec_hf[_n].copy_(env.contact_inverse_dynamics.force[:dynamics_k])
        if stance:           # (accel stays zero: the torques and wrenches that hold nu_dot = 0 on the feet the gait's phase loads)
            sd = env.stance_inverse_dynamics
            sd.stance_from_phase()
            sd.refresh()
            rec_st[_n].copy_(sd.stance[:dynamics_k])
            rec_stt[_n].copy_(sd.tau_joint[:dynamics_k])
            rec_stf[_n].copy_(sd.force[:dynamics_k])
            rec_stm[_n].copy_(sd.margins[:dynamics_k])
        if ik:               # (the feet where the policy put them, the joints from where the model starts)
            qk = env.inverse_kinematics
            qk.targets_from_bodies()
            qk.solve(q0=env.initial_dof_pos)
            rec_ikq[_n].copy_(qk.q[:dynamics_k])
            rec_ike[_n].copy_(qk.err[:dynamics_k])
            rec_ikc[_n].copy_(qk.converged[:dynamics_k])
        played = _n + 1
        cr += r.view(N)
        steps += 1
        idx = done.nonzero(as_tuple=False).view(-1)
        k = int(idx.numel())
        if k > 0:
            games_played += k
            cur_r, cur_s = float(cr[idx].sum()), float(steps[idx].sum())
            keep = 1.0 - done.float().view(N)
            cr, steps = cr * keep, steps * keep
            sum_rewards += cur_r
            sum_steps += cur_s
            print("reward:", cur_r / k, "steps:", cur_s / k, flush=True)
            if env.run_trace is not None and args.trace_hold != "never":
                traces_written = drain_held(env.run_trace, args.trace_dir, traces_written)
            if games_played >= args.games:
                break
    if args.report:
        from isaacgymdyros_amd.episode_stats import format_table
        print(format_table(env.episode_stats.summary()), flush=True)
    if env.run_trace is not None:
        if args.trace_hold == "never":
            for e in env.run_trace.env_ids:
                env.run_trace.save_npz(os.path.join(args.trace_dir, "ring_env%d.npz" % e), e)
            traces_written = len(env.run_trace.env_ids)
        print("run trace: %d files written to %s" % (traces_written, args.trace_dir), flush=True)
    if env.gait_profile is not None:
        from isaacgymdyros_amd import gait_profile as GP
        gs = env.gait_profile.summary()
        print(GP.format_table(gs), flush=True)
        if args.gait_dir:
            txt = GP.write_txt(args.gait_dir, gs)          # (creates the directory)
            GP.write_npz(os.path.join(args.gait_dir, "gait_profile.npz"), gs)
            print("gait profile: written to %s and %s" % (os.path.join(args.gait_dir, "gait_profile.npz"), txt), flush=True)
    if bodies_k:
        import numpy as np
        bs = env.body_states
        for e in range(bodies_k):
            np.savez(os.path.join(args.bodies_dir, "bodies_env%d.npz" % e), names=np.asarray(bs.names), parents=np.asarray(bs.parents, np.int32),
                     dt=np.float64(bs.dt), states=rec_states[:played, e].cpu().numpy(), com=rec_com[:played, e].cpu().numpy())
        print("body states: %d steps of %d envs written to %s" % (played, bodies_k, args.bodies_dir), flush=True)
    if scan_k:
        import numpy as np
        for e in range(scan_k):
            np.savez(os.path.join(args.scan_dir, "scan_env%d.npz" % e), grid=hsc.grid, names=np.asarray(hsc.names), dt=np.float64(hsc.dt),
                     heights=rec_hts[:played, e].cpu().numpy(), probe_pos=rec_ppos[:played, e].cpu().numpy(), clearance=rec_clr[:played, e].cpu().numpy())
        print("height scan: %d steps of %d envs written to %s" % (played, scan_k, args.scan_dir), flush=True)
    if sensors_k:
        import numpy as np
        fs = env.force_sensors
        for e in range(sensors_k):
            np.savez(os.path.join(args.sensors_dir, "sensors_env%d.npz" % e), names=np.asarray(fs.names), dt=np.float64(fs.dt),
                     sensors=rec_sen[:played, e].cpu().numpy(), cop=rec_cop[:played, e].cpu().numpy(), zmp=rec_zmp[:played, e].cpu().numpy())
        print("force sensors: %d steps of %d envs written to %s" % (played, sensors_k, args.sensors_dir), flush=True)
    if dynamics_k:
        import numpy as np
        jc = env.jacobians
        for e in range(dynamics_k):
            more = {}
            if forces:
                more = dict(bias=rec_bias[:played, e].cpu().numpy(), gravity=rec_grav[:played, e].cpu().numpy(), momentum=rec_mom[:played, e].cpu().numpy())
            if accel:
                more.update(minv=rec_minv[:played, e].cpu().numpy(), accel_zero_torque=rec_acc[:played, e].cpu().numpy())
            if contact:
                more.update(contact_jacobian=rec_cjac[:played, e].cpu().numpy(), contact_lambda=rec_clam[:played, e].cpu().numpy(),
                            contact_force_zero_torque=rec_cf[:played, e].cpu().numpy())
            if inverse:
                more.update(hold_torque=rec_ht[:played, e].cpu().numpy(), hold_force=rec_hf[:played, e].cpu().numpy())
            if stance:
                more.update(stance=rec_st[:played, e].cpu().numpy(), stance_torque=rec_stt[:played, e].cpu().numpy(),
                            stance_force=rec_stf[:played, e].cpu().numpy(), stance_margins=rec_stm[:played, e].cpu().numpy())
            if ik:
                more.update(ik_q=rec_ikq[:played, e].cpu().numpy(), ik_err=rec_ike[:played, e].cpu().numpy(), ik_converged=rec_ikc[:played, e].cpu().numpy())
            np.savez(os.path.join(args.dynamics_dir, "dynamics_env%d.npz" % e), names=np.asarray(jc.names), dof_names=np.asarray(jc.dof_names),
                     dt=np.float64(jc.dt), jacobian=rec_jac[:played, e].cpu().numpy(), mass_matrix=rec_mm[:played, e].cpu().numpy(),
                     com_jacobian=rec_cj[:played, e].cpu().numpy(), **more)
        print("dynamics: %d steps of %d envs written to %s" % (played, dynamics_k, args.dynamics_dir), flush=True)
    env.close()
    if games_played == 0:
        raise SystemExit("no game ended within --max-steps %d" % args.max_steps)
    av_r, av_s = sum_rewards / games_played, sum_steps / games_played
    print("av reward:", av_r, "av steps:", av_s, flush=True)
    if not (math.isfinite(av_r) and math.isfinite(av_s)):
        raise SystemExit("non-finite average")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--checkpoint", required=True, help="a checkpoint of examples/ppo_consumer.py --output-dir (or the reference learner's)")
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--games", type=int, default=100)
    ap.add_argument("--max-steps", type=int, default=10000)
    ap.add_argument("--stochastic", action="store_true", help="sample mu + exp(sigma) noise instead of the deterministic mu")
    ap.add_argument("--policy-backend", default="hip", choices=["hip", "torch"])
    ap.add_argument("--export-dir", default=None, help="write the model tensors as the reference's text files here")
    ap.add_argument("--episode-length", type=float, default=None, help="episode length in seconds (default: the yaml's 32 s)")
    ap.add_argument("--report", action="store_true", help="collect the on-GPU episode statistics and print their table at the end")
    ap.add_argument("--nominal", action="store_true", help="task.randomize False and env.perturbation False (encoder noise stays on)")
    ap.add_argument("--trace-dir", default=None, help="turn the on-GPU run trace on and write its rings here (fall_env<id>_<n>.npz)")
    ap.add_argument("--trace-envs", type=int, default=64, help="trace envs 0 .. K-1")
    ap.add_argument("--trace-depth", type=int, default=512, help="steps kept per traced env")
    ap.add_argument("--trace-hold", default="fall", choices=["never", "fall", "reset"],
                    help="freeze a slot at the step that ends its episode: other than by the time limit / at any reset / never")
    ap.add_argument("--gait-report", action="store_true", help="collect the on-GPU gait profile and print its three-window table at the end")
    ap.add_argument("--gait-dir", default=None, help="turn the gait profile on and write gait_profile.npz and gait_profile.txt here")
    ap.add_argument("--gait-bins", type=int, default=72, choices=[12, 24, 36, 72, 144], help="phase bins of the gait profile")
    ap.add_argument("--bodies-dir", default=None, help="turn the rigid-body state tensor on and write bodies_env<id>.npz (every body's trajectory) here")
    ap.add_argument("--bodies-envs", type=int, default=1, help="record envs 0 .. K-1")
    ap.add_argument("--scan-dir", default=None, help="turn the terrain height scan on and write scan_env<id>.npz (the heights around the base, the sole corners and their clearance) here")
    ap.add_argument("--scan-envs", type=int, default=1, help="record envs 0 .. K-1")
    ap.add_argument("--sensors-dir", default=None, help="turn the foot force-torque sensors on and write sensors_env<id>.npz (wrenches, centres of pressure, ZMP) here")
    ap.add_argument("--sensors-envs", type=int, default=1, help="record envs 0 .. K-1")
    ap.add_argument("--dynamics-dir", default=None, help="turn the Jacobian and mass-matrix tensors on and write dynamics_env<id>.npz (head and foot Jacobians, M, COM Jacobian) here")
    ap.add_argument("--dynamics-envs", type=int, default=1, help="record envs 0 .. K-1")
    ap.add_argument("--dynamics-accel", action="store_true", help="with --dynamics-dir: add the inverse of the mass matrix and the zero-torque acceleration M^-1 (-h) to each file")
    ap.add_argument("--dynamics-contact", action="store_true", help="with --dynamics-dir: add the feet's contact Jacobian, the contact-space inertia and the zero-torque ground reaction with planted feet to each file")
    ap.add_argument("--dynamics-inverse", action="store_true", help="with --dynamics-dir: add the joint torques and foot wrenches that would hold nu_dot = 0 at each played state to each file")
    ap.add_argument("--dynamics-stance", action="store_true", help="with --dynamics-dir: add the stance of the gait's phase, and the joint torques, foot wrenches and sole margins that would hold nu_dot = 0 under it, to each file")
    ap.add_argument("--dynamics-ik", action="store_true", help="with --dynamics-dir: add the joint angles that put both feet at their played poses, solved from the model's initial angles, to each file")
    ap.add_argument("--dynamics-forces", action="store_true", help="with --dynamics-dir: add the bias forces, the gravity forces and the momentum to each file")
    ap.add_argument("--device", default="cuda:0")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
