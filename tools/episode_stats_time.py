#!/usr/bin/env python3
"""Cost of the episode statistics: milliseconds per eager step() with cfg sim.mi355.episode_stats off and on, same seed
and actions, each after a warm-up.  Run under `rocprofv3 --kernel-trace --stats -- python tools/episode_stats_time.py --only-on` for
dws_k_record's own time."""
import argparse
import json

from _timing import actions, loop_ms, make_env


def run(n, steps, warmup, on):
    env = make_env(n, "episode_stats", on, alias_obs=True)
    a = actions(n)
    out = {"episode_stats": on, "num_envs": n, "ms_per_step": loop_ms(lambda t: env.step(a[t % 8]), steps, warmup)}
    if on:
        s = env.episode_stats.summary()
        out["episodes"], out["causes"] = s["episodes"], s["causes"]
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--only-on", action="store_true")
    a = ap.parse_args()
    for on in ((True,) if a.only_on else (False, True, False, True)):
        print(json.dumps(run(a.num_envs, a.steps, a.warmup, on)), flush=True)


if __name__ == "__main__":
    main()
