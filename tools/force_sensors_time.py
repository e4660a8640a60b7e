#!/usr/bin/env python3
"""Cost of the foot force-torque sensors at --num-envs envs.
  kernel: microseconds per dwf_k_refresh alone, from device events around replays of a captured chain of 100 launches (so that the host's
          launch rate does not bound it), on the buffers a real env holds after --warm-steps steps of small random actions: the default
          selection (two sensors, cop, zmp) and everything switched on (eight sensors, cop, zmp, corners).  Beside them, in the same process
          and measured the same way, alternating over --rounds rounds: dwb_k_refresh restricted to the two foot rows (it walks the same
          two leg paths: the yardstick) and a device-to-device copy of each selection's output bytes.
  step:   eager env.step() in milliseconds with force_sensors off / on / off / on ("auto": True); off is the parent commit's code path."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from _timing import DEV, make_env, step_ms
EIGHT = [{"body": b, "pos": [0.01 * i, 0.0, -0.09], "quat": q, "world_frame": w}
         for i, (b, q, w) in enumerate([("L_Foot_Link", [0, 0, 0, 1], False), ("R_Foot_Link", [0, 0, 0, 1], False), ("L_Foot_Link", [0, 0, 0.6, 0.8], False),
                                        ("R_Foot_Link", [0, 0, 0.6, 0.8], False), ("L_Foot_Link", [0, 0, 0, 1], True), ("R_Foot_Link", [0, 0, 0, 1], True),
                                        ("L_Foot_Link", [0.6, 0, 0, 0.8], False), ("R_Foot_Link", [0.6, 0, 0, 0.8], True)])]


def chain(fn, chain_len=100):
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        for _ in range(chain_len):
            fn()
    gr.replay()
    torch.cuda.synchronize()
    return gr


def replay_us(gr, launches, chain_len=100):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches // chain_len):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (launches // chain_len * chain_len) * 1e3


def kernel(n, warm_steps, launches, rounds):
    from isaacgymdyros_amd.body_states import BodyStates
    from isaacgymdyros_amd.force_sensors import ForceSensors
    env = make_env(n, "force_sensors", None)
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(warm_steps):
        env.step((torch.rand(n, 13, generator=g, device=DEV) * 2 - 1) * 0.05)
    loaded = float((env._buf["env_state"][:, 344:368].reshape(n, 8, 3)[..., 2] > 0).float().mean())
    cases = []
    for what, spec in (("default: 2 sensors + cop + zmp", {}), ("all: 8 sensors + cop + zmp + corners", {"sensors": EIGHT, "corners": True})):
        fs = ForceSensors(env, spec)
        words = sum(t.numel() for t in (fs.sensors, fs.cop, fs.zmp, fs.corners) if t is not None)
        src, dst = torch.rand(words, device=DEV), torch.empty(words, device=DEV)
        cases.append(("dwf_k_refresh", what, 4 * words, chain(fs.refresh), fs))
        cases.append(("d2d copy", "the bytes of " + what, 4 * words, chain(lambda dst=dst, src=src: dst.copy_(src)), (src, dst)))
    bs = BodyStates(env, {"bodies": ["L_Foot_Link", "R_Foot_Link"], "com": False})
    cases.append(("dwb_k_refresh", "the two foot rows", 4 * bs.states.numel(), chain(bs.refresh), bs))
    times = {i: [] for i in range(len(cases))}
    for _ in range(rounds):          # alternating: every case once per round
        for i, c in enumerate(cases):
            times[i].append(replay_us(c[3], launches))
    out = [{"kernel": c[0], "num_envs": n, "outputs": c[1], "output_bytes": c[2], "us_per_launch_in_a_captured_chain": sorted(times[i])[len(times[i]) // 2],
            "min_us": min(times[i]), "max_us": max(times[i]), "rounds": rounds, "share_of_corners_loaded": loaded} for i, c in enumerate(cases)]
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm-steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "force_sensors_time.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("force_sensors_time.py needs the GPU: a CPU run gives no time")
    rows = kernel(a.num_envs, a.warm_steps, 2000, a.rounds)
    for _ in range(2):
        for spec in (None, {"auto": True}):
            rows.append(step_ms(a.num_envs, "force_sensors", spec, 500, 50, flag=True))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# tools/force_sensors_time.py --num-envs %d --rounds %d --warm-steps %d on one MI355X (median of the rounds; min and max beside it)\n"
                % (a.num_envs, a.rounds, a.warm_steps))
        for row in rows:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
