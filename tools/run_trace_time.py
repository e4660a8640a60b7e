#!/usr/bin/env python3
"""Cost of the run trace at --num-envs envs: microseconds per dwt_k_record alone (device events around replays of a
captured chain of 100 launches on the buffers a step left, so that the host's launch rate does not bound it) for K = 64 and K = all envs, and
milliseconds per eager step() with cfg sim.mi355.run_trace off and on, same seed and actions, each after a warm-up.  The timed traces never hold:
a held slot only counts, and with hold "fall" every slot is held after a few hundred steps of random actions.  Run under
`rocprofv3 --kernel-trace --stats -- python tools/run_trace_time.py --only-on [--slots K]` for the kernel's own time within a step."""
import argparse
import json

from _timing import actions, chain_us, loop_ms, make_env


def run(n, steps, warmup, trace):
    env = make_env(n, "run_trace", trace, alias_obs=True)
    a = actions(n)
    out = {"run_trace": trace or None, "num_envs": n, "ms_per_step": loop_ms(lambda t: env.step(a[t % 8]), steps, warmup)}
    if trace:
        r = env.run_trace
        out["held"], out["ring_MB"] = int(r.held().sum()), r.ring.numel() * 4 / 1e6
    env.close()
    return out


def kernel(n, k, depth, launches):
    """dwt_k_record alone on the buffers a few steps left; hold never, so every launch writes K rows."""
    from isaacgymdyros_amd.run_trace import ROW_BYTES
    env = make_env(n, "run_trace", {"env_ids": k, "depth": depth, "hold": "never"}, alias_obs=True)
    for a in actions(n):
        env.step(a)
    us = chain_us(env.run_trace.record, launches)
    # bytes per slot: the row out, and in the 13 + 66 + 114 + 16 words the row comes from, the env_state spans (33 + 37 + 13 + 12 + 2 + 1 + 3
    # words) and the two flags
    moved = k * (ROW_BYTES + 4 * (13 + 66 + 114 + 16 + 101) + 16)
    env.close()
    return {"kernel": "dwt_k_record", "num_envs": n, "slots": k, "depth": depth, "us_per_launch_in_a_captured_chain": us, "bytes": moved,
            "GB_per_s": moved / us / 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--only-on", action="store_true")
    ap.add_argument("--slots", type=int, default=64, help="with --only-on: traced envs")
    a = ap.parse_args()
    n = a.num_envs
    small, full = {"env_ids": min(64, n), "depth": 512, "hold": "never"}, {"env_ids": n, "depth": a.depth, "hold": "never"}
    if a.only_on:
        print(json.dumps(run(n, a.steps, a.warmup, {"env_ids": min(a.slots, n), "depth": a.depth, "hold": "never"})), flush=True)
        return
    for k in (min(64, n), n):
        print(json.dumps(kernel(n, k, a.depth, 2000)), flush=True)
    for trace in (None, small, full, None, small, full):
        print(json.dumps(run(n, a.steps, a.warmup, trace)), flush=True)


if __name__ == "__main__":
    main()
