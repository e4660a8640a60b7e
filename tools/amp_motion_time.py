"""Times TocabiAMPLower's reset_done() + step() back to back, and one fetch_amp_obs_demo, with stateInit 'Random' on the synthetic motion
tables -- the configuration the task's yaml trains with.

  python tools/amp_motion_time.py --form device    fused step (hipGraph), sim.mi355.amp_motion_device + amp_device_draws: the reset is
                                                   dw_amp_reset_done_motion, the fetch one dw_amp_motion_obs launch
  python tools/amp_motion_time.py --form torch     fused step (hipGraph), torch reset on the host motion library: what the same cfg runs
                                                   without the key (also runs on a commit that has no such key)
Prints one JSON line; --out appends it to a file.  Device events around `--steps` calls after `--warmup`; a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/amp_motion_time.py --form device --steps 50` lists the launches of the window."""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=["device", "torch"], default="device")
    ap.add_argument("--num_envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--demo", type=int, default=4096)
    ap.add_argument("--episode_length", type=int, default=200, help="short episodes: a few per cent of the envs reset at every call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    from tests import amp_motion_synth as SY
    yml = SY.write(tempfile.mkdtemp(prefix="amp_synth_"))
    cfg = default_amp_cfg(a.num_envs, "cuda:0")
    cfg["env"].update({"stateInit": "Random", "motion_file": yml, "episodeLength": a.episode_length})
    cfg["sim"]["mi355"] = {"amp_fused": True}
    if a.form == "device":
        cfg["sim"]["mi355"].update({"amp_motion_device": True, "amp_device_draws": True})
    env = TocabiAMPLower(cfg, "cuda:0", 0, True)
    env.reset_done()
    env.enable_graph_step(warmup=3)
    act = torch.zeros(a.num_envs, 12, device="cuda")
    # (stagger the episodes so that resets arrive at every call rather than all at once)
    env.progress_buf.copy_(torch.randint(0, a.episode_length, (a.num_envs,), device="cuda"))
    resets = 0

    def run(k):
        n = 0
        for _ in range(k):
            n += len(env.reset_done()[1])
            env.step(act)
        return n
    run(a.warmup)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    resets = run(a.steps)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.steps
    for _ in range(5):
        env.fetch_amp_obs_demo(a.demo)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(50):
        env.fetch_amp_obs_demo(a.demo)
    t1.record()
    torch.cuda.synchronize()
    res = {"tool": "amp_motion_time", "form": a.form, "num_envs": a.num_envs, "state_init": "Random", "steps": a.steps,
           "reset_done_plus_step_ms": round(ms, 4), "env_steps_per_s": round(a.num_envs / ms * 1e3), "resets_per_call": round(resets / a.steps, 1),
           "fetch_amp_obs_demo_%d_ms" % a.demo: round(t0.elapsed_time(t1) / 50, 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
    env.close()


if __name__ == "__main__":
    main()
