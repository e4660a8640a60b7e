#!/usr/bin/env python3
"""Cost of the terrain height scan at --num-envs envs on the default trimesh terrain, every figure --reps times.
  kernel: microseconds per dwh_k_scan alone, from device events around replays of a captured chain of 100 launches (so that the host's
          launch rate does not bound it), on the buffers a real env holds after --warm-steps steps of small random actions: the default grid
          alone, the probes alone, both, and P at the cap.  Beside each, measured the same way in the same process, a device-to-device copy
          of the same number of output bytes (the yardstick for a store stream); once, dwb_k_refresh on the two foot rows (the floor of the
          probes' chain walk).
  today:  the path without the feature, eager on the same device: the reference's get_heights written in torch (some fifteen launches), and
          for the soles dwb_refresh of the two feet plus a bilinear lookup in torch; the one launch beside them, eager too.
  step:   eager env.step() in milliseconds with height_scan absent / {"auto": True}, alternating; absent is the parent commit's code path.
--kernel-only stops after the kernel rows (the run rocprofv3 --kernel-trace --stats wraps)."""
import argparse
import json

import torch

from _timing import DEV, chain_us, eager_us


def make_env(n, spec):
    from isaacgymdyros_amd.config import default_cfg, with_terrain
    from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk
    cfg = with_terrain(default_cfg(n, DEV), mesh_type="trimesh")
    if spec is not None:
        cfg["sim"]["mi355"]["height_scan"] = spec
    return DyrosDynamicWalk(cfg, DEV, 0, True)


def spread(xs):
    return {"mean": sum(xs) / len(xs), "min": min(xs), "max": max(xs)}


def get_heights_torch(root, points3, hs, border, hscale, vscale):
    """The reference's quat_apply_yaw, quat_apply and get_heights, eager."""
    N, P = points3.shape[:2]
    q = root[:, 3:7].clone().view(-1, 4)
    q[:, :2] = 0.0
    q = q / q.norm(p=2, dim=-1).clamp(min=1e-9, max=None).unsqueeze(-1)
    a, b = q.repeat(1, P).reshape(-1, 4), points3.reshape(-1, 3)
    xyz = a[:, :3]
    t = xyz.cross(b, dim=-1) * 2
    pts = (b + a[:, 3:] * t + xyz.cross(t, dim=-1)).view(N, P, 3) + root[:, :3].unsqueeze(1)
    pts += border
    pts = (pts / hscale).long()
    px = torch.clip(pts[:, :, 0].view(-1), 0, hs.shape[0] - 2)
    py = torch.clip(pts[:, :, 1].view(-1), 0, hs.shape[1] - 2)
    return torch.min(hs[px, py], hs[px + 1, py + 1]).view(N, -1) * vscale


def sole_clearance_torch(bs, corners, feet, hs, border, hscale, vscale):
    """dwb_refresh of the two feet, then the corners' world positions and a bilinear lookup under them, eager."""
    st = bs.refresh()
    q, x = st[:, feet, 3:7], st[:, feet, 0:3]          # [N, 8, 4], [N, 8, 3]
    t = torch.cross(q[..., :3], corners, dim=-1) * 2
    pos = x + corners + q[..., 3:] * t + torch.cross(q[..., :3], t, dim=-1)
    u = ((pos[..., 0] + border) / hscale).clamp(0, hs.shape[0] - 1 - 1e-3)
    v = ((pos[..., 1] + border) / hscale).clamp(0, hs.shape[1] - 1 - 1e-3)
    i, j = u.long(), v.long()
    a, b = u - i, v - j
    h = vscale * ((1 - a) * ((1 - b) * hs[i, j] + b * hs[i, j + 1]) + a * ((1 - b) * hs[i + 1, j] + b * hs[i + 1, j + 1]))
    return pos[..., 2] - h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm-steps", type=int, default=200)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    from isaacgymdyros_amd import height_scan as H
    from isaacgymdyros_amd.body_states import BodyStates
    n = a.num_envs
    env = make_env(n, None)
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(a.warm_steps):
        env.step((torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * 0.05)
    c = env._ccfg
    print(json.dumps({"map": [int(c.terrain_rows), int(c.terrain_cols)], "map_bytes": 2 * int(c.terrain_rows) * int(c.terrain_cols), "num_envs": n}), flush=True)
    cap = H.mesh(torch.linspace(-1.55, 1.55, 32).numpy(), torch.linspace(-1.55, 1.55, 32).numpy())
    scans = {}
    for what, spec, outs in (("grid 140", {"probes": None}, ("heights",)), ("probes 8", {}, ("probe_pos", "probe_heights", "clearance")),
                             ("grid 140 + probes 8", {}, ("heights", "probe_pos", "probe_heights", "clearance")),
                             ("grid 1024", {"probes": None, "grid": cap.tolist()}, ("heights",))):
        hs = H.HeightScan(env, spec)
        if "heights" not in outs:
            args = list(hs._args)
            args[12] = None          # (no heights)
            hs._args = tuple(args)
        scans[what] = hs
        words = sum(getattr(hs, o).numel() for o in outs)
        src, dst = torch.rand(words, device=DEV), torch.empty(words, device=DEV)
        us = [chain_us(hs.refresh, 2000) for _ in range(a.reps)]
        cp = [chain_us(lambda: dst.copy_(src), 2000) for _ in range(a.reps)]
        print(json.dumps({"kernel": "dwh_k_scan", "outputs": what, "output_bytes": 4 * words, "us_per_launch_in_a_captured_chain": spread(us),
                          "d2d_copy_of_the_same_bytes_us": spread(cp), "ratio_to_the_copy": spread(us)["mean"] / spread(cp)["mean"]}), flush=True)
    bs = BodyStates(env, {"bodies": ["L_Foot_Link", "R_Foot_Link"], "com": False})
    print(json.dumps({"kernel": "dwb_k_refresh", "outputs": "the two foot rows", "us_per_launch_in_a_captured_chain": spread([chain_us(bs.refresh, 2000) for _ in range(a.reps)])}), flush=True)
    if a.kernel_only:
        env.close()
        return
    both = scans["grid 140 + probes 8"]
    margs = (env.height_samples, float(c.terrain_border), float(c.terrain_hscale), float(c.terrain_vscale))
    pts = torch.zeros(n, 140, 3, device=DEV)
    pts[:, :, :2] = torch.from_numpy(both.grid).to(DEV)
    corners = torch.tensor([p["pos"] for p in both.probes], device=DEV).unsqueeze(0)
    feet = [0, 0, 0, 0, 1, 1, 1, 1]
    root = env._buf["root_states"]
    rows = {"one launch, grid + probes (eager)": lambda: both.refresh(), "one launch, grid (eager)": lambda: scans["grid 140"].refresh(),
            "today: get_heights in torch": lambda: get_heights_torch(root, pts, *margs),
            "today: dwb_refresh + torch bilinear for the soles": lambda: sole_clearance_torch(bs, corners, feet, *margs)}
    for what, fn in rows.items():
        print(json.dumps({"eager": what, "us_per_call": spread([eager_us(fn, 300) for _ in range(a.reps)])}), flush=True)
    env.close()
    for _ in range(a.reps):
        for spec in (None, {"auto": True}):
            env = make_env(n, spec)
            act = (torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * 0.05
            for _ in range(50):
                env.step(act)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(500):
                env.step(act)
            e1.record()
            torch.cuda.synchronize()
            env.close()
            print(json.dumps({"eager_step": True, "height_scan": spec is not None, "num_envs": n, "steps": 500, "ms_per_step": e0.elapsed_time(e1) / 500}), flush=True)


if __name__ == "__main__":
    main()
